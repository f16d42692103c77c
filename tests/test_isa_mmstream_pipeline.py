"""Guards on the stage loop of the streaming GEMM (k_mmstream, k_mmstream_p; no GPU needed: hipcc cross-compiles evalmm.hip).

The ring of digit-fragment reads runs on from one 256-row stage into the next, so the stage's ONE barrier sits in the middle of the stage (behind slot
2 CH + CH - 1 - DEPTH = 41 of 64: csrc/evalmm.hip, at the barrier) instead of at its end, waits for the wave's own ds_writes only, and is not followed by a refill of the
ring.  What the source cannot promise and the compiler has undone before: the order of the LDS operations around the barrier, and the s_waitcnt at the head of the loop
(the minimum over the paths into it: a prologue that fills the ring in another order drains it once per stage)."""
import re

import pytest

from test_isa_regressions import _asm_of, _kernel, _mfma_loop

# what csrc/evalmm.hip builds with its defaults (SW = 8 waves, RQ = 2 row tiles per wave, DEPTH = 6)
CH, DEPTH, BPK, RQ = 16, 6, 2, 2
READS_BEHIND_WRITE = CH - DEPTH - BPK          # ring reads between the barrier k-step's last ds_write and the barrier: the lgkmcnt the barrier waits for
MFMAS_BEHIND_WRITE = RQ * READS_BEHIND_WRITE   # 16 MFMAs between that ds_write and the barrier: its latency is not waited for

KERNELS = ["_ZN12_GLOBAL__N_110k_mmstreamE", "_ZN12_GLOBAL__N_112k_mmstream_pE"]


@pytest.fixture(scope="module")
def asm_evalmm(tmp_path_factory):
    return _asm_of(tmp_path_factory, "evalmm")


@pytest.fixture(scope="module", params=KERNELS)
def loop(request, asm_evalmm):
    lp = _mfma_loop(_kernel(asm_evalmm, request.param), 128)
    assert sum("v_mfma" in x for x in lp) == 128  # one stage per iteration
    return lp


def _barrier(loop):
    at = [i for i, x in enumerate(loop) if x.startswith("s_barrier")]
    assert len(at) == 1, at
    return at[0]


def test_one_barrier_per_stage(loop):
    _barrier(loop)


def test_the_ring_is_not_refilled_behind_the_barrier(loop):
    """at most one ds_read_b128 between the barrier and the next MFMA (six when the ring restarted from empty behind a barrier at the stage's end)"""
    k = _barrier(loop)
    nxt = next(i for i in range(k + 1, len(loop)) if "v_mfma" in loop[i])
    assert sum(x.startswith("ds_read_b128") for x in loop[k + 1:nxt]) <= 1, loop[k:nxt + 1]
    # and none in front of the stage's first MFMA: the fragments it needs were read by the previous stage
    first = next(i for i, x in enumerate(loop) if "v_mfma" in x)
    assert not any(x.startswith("ds_read") for x in loop[:first]), loop[:first + 1]


def test_the_barrier_waits_for_the_ds_writes_only_and_far_behind_them(loop):
    k = _barrier(loop)
    m = re.match(r"s_waitcnt lgkmcnt\((\d+)\)$", loop[k - 1])
    assert m and int(m.group(1)) == READS_BEHIND_WRITE, loop[k - 3:k + 1]
    w = max(i for i, x in enumerate(loop[:k]) if x.startswith("ds_write"))
    between = loop[w + 1:k]
    assert sum("v_mfma" in x for x in between) >= MFMAS_BEHIND_WRITE, sum("v_mfma" in x for x in between)
    # the hand-written count is exact only if these are the LDS operations behind the last ds_write, and nothing else shares the counter
    assert sum(x.startswith("ds_read_b128") for x in between) == READS_BEHIND_WRITE
    assert not any(x.startswith(("s_load", "s_buffer_load", "ds_write")) for x in between)


def test_no_wait_of_the_loop_drains_the_ring(loop):
    """no s_waitcnt of the stage loop asks for fewer LDS operations in flight than DEPTH - 1: the reads stay ahead of the MFMAs through the whole stage, its head included"""
    waits = [int(m.group(1)) for x in loop for m in [re.search(r"lgkmcnt\((\d+)\)", x)] if m]
    assert waits and min(waits) >= DEPTH - 1, waits
    assert not any(x.startswith(("s_load", "s_buffer_load")) for x in loop)  # (scalar loads return out of order: every count would mean 0)


def test_stage_loop_shape(loop):
    assert not any(x.startswith("scratch_") for x in loop)
    assert sum(x.startswith("global_load_dwordx4") for x in loop) == 16
    assert sum(x.startswith("ds_read_b128") for x in loop) == 64
    assert sum(x.startswith("ds_write_b128") for x in loop) == 8
