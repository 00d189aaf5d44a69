"""Exit probe of the per-bounce trace kernel: frame time of one scene, and with --probe one profiled frame whose trace launches
print when their wavefronts start, start their last batch and run out of work (options `exit_probe` + `debug_levels`).
usage: python profiles/exit_probe.py [scene] [WxH] [shard] [--probe]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ndt_amd import load_scene
from ndt_amd.hip import NdtHip

args = [a for a in sys.argv[1:] if not a.startswith("--")]
scene = args[0] if args else "c3_random4d"
w, h = (int(x) for x in (args[1] if len(args) > 1 else "1920x1080").split("x"))
shard = int(args[2]) if len(args) > 2 else 1
fs = load_scene("tests/golden/%s.ndtscene.gz" % scene)
g = NdtHip(0)
g.upload_scene(fs)
g.set_option("pipeline", 1)
rows = (h + shard - 1) // shard
buf = torch.empty((rows, w, 4), dtype=torch.float64, device="cuda")
if "--probe" in sys.argv:
    g.set_option("exit_probe", 1)
    g.set_option("debug_levels", 1)
for _ in range(3):
    g.render_device(buf.data_ptr(), w, h, 4, row_begin=0, row_step=shard)
torch.cuda.synchronize()
best = 1e9
for rep in range(3):
    t0 = time.perf_counter()
    n = 20
    for _ in range(n):
        st = g.render_device(buf.data_ptr(), w, h, 4, row_begin=0, row_step=shard)
    torch.cuda.synchronize()
    best = min(best, 1e3 * (time.perf_counter() - t0) / n)
print("%s %dx%d r::%d: %.3f ms a frame" % (scene, w, h, shard, best), flush=True)
if "--probe" in sys.argv:
    sys.stderr.flush()
    st = g.render_device(buf.data_ptr(), w, h, 4, row_begin=0, row_step=shard, profile=1)
    print("   profiled: frame %.3f ms, trace %.3f ms in %d launches" % (st.frame_ms, st.trace_ms, st.trace_launches), flush=True)
