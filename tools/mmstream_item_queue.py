"""Where a persistent streaming launch ends: per-XCD end times of the workgroups of k_mmstream_p / k_mmstream_pb in one mfh_prove_batch step. dev tool.

Needs a DIAGNOSTIC build of libmfhip.so (csrc/evalmm.hip compiled with -DMMS_ITEM_STAMPS, loaded through $MFHIP_LIB): wave 0 of every workgroup stamps s_memrealtime
(100 MHz) at the entry of its first item, when it leaves its last item and when that item's stores have landed, and counts its items.  Such a build is never timed for
a headline figure.

build: tools/build_mm_variants.sh stamps "-DMMS_ITEM_STAMPS"          (tools/ab/libmfhip_mm_stamps.so)
usage: MFHIP_LIB=<diagnostic build> python tools/mmstream_item_queue.py [MODE[:PREFIX] ...]     (default: 0; e.g. "0 1 1:0" = static walk, queue, queue without prefix)
Per mode: two warm-up steps of $BATCH_PROF_NB (default 1020) statements, then one step whose launches are printed: per XCD the minimum, mean and maximum end time of
its 32 workgroups relative to the launch's earliest entry, the items they ran (and how many of them came from a foreign XCD's queue), the mean item time and
launch / mean item time."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import c_lwe_snarks_amd as mf

TICK_US = 0.01  # s_memrealtime counts at 100 MHz


def read_stamps(lib):
    buf = (ctypes.c_ulonglong * (64 * 257 * 4))()
    lib.mfh_mm_item_stamps.restype = ctypes.c_uint32
    lib.mfh_mm_item_stamps.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    n = lib.mfh_mm_item_stamps(buf, 64)
    a = np.frombuffer(buf, dtype=np.uint64).reshape(64, 257, 4)[:n].copy()
    return [(int(l[0, 0]) & 0xFF, int(l[0, 0]) >> 8, l[1:]) for l in a]


def report(tag, launches):
    for i, (nd, queue, st) in enumerate(launches):
        items = (st[:, 3] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        foreign = (st[:, 3] >> np.uint64(32)).astype(np.int64)
        ran = items > 0
        t0 = int(st[ran, 0].min())
        first = (st[:, 0].astype(np.int64) - t0) * TICK_US
        left = (st[:, 1].astype(np.int64) - t0) * TICK_US    # wave 0 leaves its last item (stores issued)
        landed = (st[:, 2].astype(np.int64) - t0) * TICK_US  # ... and they have landed (behind the failed claims, with the queue)
        busy = (left - first)[ran].sum()
        item_us = busy / items.sum()
        launch_us = left[ran].max()
        name = "k_mmstream_pb" if nd == 1 else "k_mmstream_p"
        print(f"## {tag} launch {i} {name} queue={queue}: {int(ran.sum())} workgroups, {int(items.sum())} items ({int(foreign.sum())} from a foreign queue), "
              f"mean item {item_us:.2f} us, launch (earliest entry -> last workgroup leaves) {launch_us:.1f} us = {launch_us / item_us:.3f} item times; "
              f"stores landed by {landed[ran].max():.1f} us; entries spread over {first[ran].max():.1f} us")
        print("#  xcd  items(min..max)  foreign  end min      mean       max   (us after the earliest entry)   per-item time of the XCD's workgroups")
        for x in range(8):
            sel = ran & (np.arange(256) % 8 == x)
            if not sel.any():
                continue
            per = ((left - first)[sel] / items[sel]).mean()
            print(f"   {x}    {items[sel].min():3d} .. {items[sel].max():3d}      {foreign[sel].sum():5d}  {left[sel].min():9.1f} {left[sel].mean():9.1f} {left[sel].max():9.1f}"
                  f"                                   {per:8.2f}")


def main():
    modes = sys.argv[1:] or ["0"]
    p = mf.DEFAULT
    ctx = mf.Context(p, 0)
    lib = ctx.lib
    if not hasattr(lib, "mfh_mm_item_stamps"):
        raise SystemExit("this libmfhip.so is not a diagnostic build (-DMMS_ITEM_STAMPS); point $MFHIP_LIB at one")
    ctx.set_seed(bytes((37 * i + 11) & 0xFF for i in range(40)))
    inst = bench.build_instance(mf, ctx, torch, p, 20260101)
    ctx.ssp_prepare(inst["d_ssp"])
    d_crs = ctx.setup(inst["d_ssp"], inst["alpha"], inst["beta"], inst["s"], inst["sk"], inst["err"])
    rng = np.random.default_rng(5)
    nb = int(os.environ.get("BATCH_PROF_NB", "1020"))
    deltas = [int(x) for x in rng.integers(0, mf.P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(5)] * nb
    out = None
    for m in modes:
        mode, _, prefix = m.partition(":")
        ctx.set_mm_queue(int(mode), 0, int(prefix) if prefix else -8)
        for _ in range(2):
            out = ctx.prove_batch(d_crs, inst["d_ssp"], [inst["bits"]] * nb, deltas, mags, signs, out=out)
        read_stamps(lib)  # (waits for the device and starts over)
        out = ctx.prove_batch(d_crs, inst["d_ssp"], [inst["bits"]] * nb, deltas, mags, signs, out=out)
        report(f"mode {m}", read_stamps(lib))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
