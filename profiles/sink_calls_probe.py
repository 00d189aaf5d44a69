"""Every host-memory and file sink of tests/golden/make_golden_sinks.py's matrix once, at 64 x 36, one context a stage -- the
program of profiles/sink_delivery.md's API-call table:

    rocprofv3 --hip-trace --stats -d <dir> -o sinks --output-format csv -- python profiles/sink_calls_probe.py

and, without the profiler, the host times the library reports for the delivery itself: ndt_hip_depth_ms() and the encode time of
the file's record.  Single small-frame figures: what they hold is launch and copy latency.
"""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_sinks", os.path.join(HERE, "..", "tests", "golden", "make_golden_sinks.py"))
matrix = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(matrix)
matrix.W, matrix.H = 64, 36


def main():
    from ndt_amd.hip import NdtHip
    scene, depth = matrix._scene()
    entries = [e for e in matrix.ENTRIES if e.kind != "device"]
    for stage in dict.fromkeys(e.stage for e in entries):
        gpu = NdtHip(0)
        gpu.set_option("sample_seed", matrix.SEED)
        gpu.upload_scene(scene)
        for e in entries:
            if e.stage != stage:
                continue
            gpu.png_stats = gpu.jpeg_stats = gpu.exr_stats = gpu.apng_stats = None
            e.good(gpu, depth, {})
            times = ["depth_ms %.3f" % gpu.lib.ndt_hip_depth_ms(gpu.ctx)] if "depth" in e.name else []
            for name, field in (("png_stats", "encode_ms"), ("jpeg_stats", "encode_ms"), ("exr_stats", "ms"), ("apng_stats", "encode_ms")):
                st = getattr(gpu, name)
                if st is not None:
                    records = st if hasattr(st, "__len__") else [st]
                    times.append("%s %s" % (name, " ".join("%.3f" % getattr(r, field) for r in records)))
            print("%-28s %s" % (e.name, "  ".join(times)), flush=True)
        gpu.close()


if __name__ == "__main__":
    main()
