"""Measurements of the animated-PNG path; its output is committed in profiles/apng_on_device.txt.

Input: a directory of the still files `ndt_hip ... -f a:b --png --deflate gpu` wrote for a run (and, optionally, the `.apng` the
same run wrote with `--apng`).  The stills are decoded here (Python's zlib) into the run's 8-bit frames, which are uploaded once;
then, per frame and alternating, the still encoder (ndt_hip_encode_png_device) and the animation's add (ndt_hip_apng_add_device)
run on the same device image, `runs` sessions after one warm-up session; encode_ms is each call's own host clock, launch to the
bytes in host memory.  Reported: per frame the rectangle, the bytes of both and the median times; the file's size against the sum
of the stills.  The still encoder's bytes are compared with the files, so a library other than the one that wrote them
(NDT_HIP_LIB; one without the animation's entry points gets the still figures alone) is shown to write the same files.
Usage: python profiles/apng_probe.py STILLS_DIR [FILE.apng] [runs]"""
import glob
import os
import statistics
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_amd import hip as nh      # noqa: E402


def inflate(png):
    """pixels [h, w, 4] of a one-IDAT 8-bit RGBA PNG with filters 0 / 1 / 2"""
    w, h = struct.unpack(">II", png[16:24])
    n, = struct.unpack(">I", png[33:37])
    assert png[37:41] == b"IDAT" and zlib.crc32(png[37:41 + n]) == struct.unpack(">I", png[41 + n:45 + n])[0]
    raw = np.frombuffer(zlib.decompress(png[41:41 + n]), dtype=np.uint8).reshape(h, 1 + 4 * w)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, 4)
        out[r] = np.cumsum(row, axis=0, dtype=np.uint8) if raw[r, 0] == 1 else row + out[r - 1] if raw[r, 0] == 2 and r else row
    return out


def main():
    import torch
    args = sys.argv[1:]
    paths = sorted(glob.glob(os.path.join(args[0], "*.png")))
    apng_path = args[1] if len(args) > 1 and not args[1].isdigit() else None
    runs = int(args[-1]) if len(args) > 1 and args[-1].isdigit() else 11
    stills = [open(p, "rb").read() for p in paths]
    frames = [inflate(s) for s in stills]
    h, w, _ = frames[0].shape
    gpu = nh.NdtHip(0)
    have = hasattr(gpu.lib, "ndt_hip_apng_add_device")
    print("library %s (%s the animation's entry points), %d frames of %dx%d from %s, %d sessions after 1 warm-up" % (
        os.path.basename(os.path.dirname(nh.LIB_PATH)) + "/" + os.path.basename(nh.LIB_PATH), "with" if have else "without", len(frames), w, h,
        args[0], runs))
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    t_png = [[] for _ in frames]
    t_add = [[] for _ in frames]
    rec = [None] * len(frames)
    total = 0
    for run in range(runs + 1):
        if have:
            gpu.apng_begin(w, h, len(frames))
        total = 0
        for k, d in enumerate(dev):
            png = gpu.encode_png_device(d.data_ptr(), w, h)
            assert png == stills[k], "frame %d: the still encoder's bytes are not the file's" % k
            ms_png = gpu.png_stats.encode_ms
            if have:
                part = gpu.apng_add_device(d.data_ptr())
                st = gpu.apng_stats
                rec[k] = (st.w, st.h, st.x, st.y, st.blend, st.changed, st.translucent, len(part), st.launches)
                total += len(part)
                if run:
                    t_add[k].append(st.encode_ms)
            if run:
                t_png[k].append(ms_png)
        if have:
            total += len(gpu.apng_end())
    med_png = [statistics.median(t) for t in t_png]
    print("still encoder, encode_ms per frame: median of the frames' medians %.3f [min %.3f .. max %.3f]; the %d files %d bytes" % (
        statistics.median(med_png), min(med_png), max(med_png), len(stills), sum(len(s) for s in stills)))
    if not have:
        return
    med_add = [statistics.median(t) for t in t_add]
    for k in range(len(frames)):
        r = rec[k]
        print("frame %2d: %4d x %4d at %4d,%4d blend %d, %7d changed (%d translucent): %7d bytes in %d launches (still %7d); "
              "encode_ms add %.3f [%.3f .. %.3f], still %.3f [%.3f .. %.3f]" % (
                  k, r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], len(stills[k]), med_add[k], min(t_add[k]), max(t_add[k]),
                  med_png[k], min(t_png[k]), max(t_png[k])))
    later_add, later_png = med_add[1:] or med_add, med_png[1:] or med_png
    print("animation's add, encode_ms per frame: frame 0 %.3f; later frames median %.3f [min %.3f .. max %.3f]; ratio of the later frames' "
          "medians add / still: %.3f" % (med_add[0], statistics.median(later_add), min(later_add), max(later_add),
                                         statistics.median(later_add) / statistics.median(later_png)))
    stills_sum = sum(len(s) for s in stills)
    print("size: the animated file %d bytes, the %d stills %d bytes: x%.3f" % (total, len(stills), stills_sum, total / stills_sum))
    if apng_path:
        on_disk = os.path.getsize(apng_path)
        print("the driver's file %s: %d bytes (%s)" % (os.path.basename(apng_path), on_disk, "the same" if on_disk == total else "DIFFERENT"))
    gpu.close()


if __name__ == "__main__":
    main()
