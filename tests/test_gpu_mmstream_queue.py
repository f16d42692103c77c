"""The item queues of the persistent streaming GEMM (csrc/evalmm.hip: mmstream_persistent under k_mmstream_p and k_mmstream_pb; mfh_set_mm_queue).

With the queues a workgroup no longer walks a fixed list of (group, tile group, chunk) items: it runs a static prefix of that list, then claims items from its XCD's
counter and, when that queue is exhausted, from the other XCDs'.  An item computes what it computed before -- only who runs it changes -- so every case compares the
proofs BYTE FOR BYTE with the regenerating path (set_batch_image(False): no streaming kernel at all), computed once per instance, and reads the claim log
(mfh_set_mm_claim_log): every item that exists was taken exactly once, every slot without a tile group never, and the owners are who the mode says they are.

Instances as in tests/test_gpu_mmstream_pipeline.py: d in {256, 512, 1024} (1, 2, 4 stages per item), m = 300, 70 statements; 300 statements = two super-groups, whose b_w is
ONE k_mmstream_pb launch over m = 341 rows.  70 statements are THREE groups per region, and neither three nor six divides 32, so their S / AS launch is one workgroup per
item (k_mmstream), not the persistent grid: those cases pin the bytes in every mode and have an empty claim log.  Every shape is therefore run with 100 statements as well
(four groups per region, eight per launch: the persistent grid), and there the log must not be empty."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes((11 * i + 3) & 0xFF for i in range(40))
LOG_WORDS = 1 << 20
DEFAULT = (1, 0, -8)  # the library's own (mode, start_shift, prefix): csrc/ctx.hpp
STATIC = 0xFF  # the `from` field of an item a workgroup took from its static list


def _statements(rng, p, n, valid_bits):
    nbytes = (p.m + 7) // 8
    bits = [valid_bits if b % 3 != 2 else rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for b in range(n)]
    deltas = [int(x) for x in rng.integers(0, ol.P, size=n, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(n)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(n)]
    return bits, deltas, mags, signs


def _item(xcd, slot, ngt, ngr, map_):
    """the static map (csrc/mms_slots.hpp: mms_item), restated: slot of an XCD -> (group, tile group)"""
    if map_ == 0:
        return slot % ngt, (slot // ngt) * 8 + xcd
    blk, i, nreg, tpb = slot >> 5, slot & 31, ngt // ngr, 32 // ngr
    return (blk % nreg) * ngr + i % ngr, ((blk // nreg) * tpb + i // ngr) * 8 + xcd


class _Launch:
    """one persistent launch of a logged call: its shape, how often each (chunk, XCD, slot) was taken, by which workgroup and from which queue"""

    def __init__(self, desc, words):
        self.__dict__.update(desc)
        self.per_chunk = self.nblk * 32
        sec = words[self.offset:self.offset + 2 * self.nchunks * 8 * self.per_chunk].reshape(self.nchunks, 8, self.per_chunk, 2)
        self.count = sec[..., 0].astype(np.int64)
        self.block = (sec[..., 1] & 0xFFFF).astype(np.int64) - 1  # blockIdx.x of the owner (-1: nobody)
        self.src = (sec[..., 1] >> 16).astype(np.int64)
        self.valid = np.zeros((8, self.per_chunk), dtype=bool)
        for x in range(8):
            for s in range(self.per_chunk):
                self.valid[x, s] = _item(x, s, self.ngt, self.ngr, self.map)[1] < self.tgs
        self.xcd = np.broadcast_to(np.arange(8)[None, :, None], self.count.shape)
        self.slot = np.broadcast_to(np.arange(self.per_chunk)[None, None, :], self.count.shape)
        self.flat = self.slot + self.per_chunk * np.arange(self.nchunks)[:, None, None]

    def check_exactly_once(self):
        assert np.array_equal(self.count, np.broadcast_to(self.valid[None], self.count.shape).astype(np.int64))
        assert (self.block[self.count == 0] == -1).all()

    def check_owners(self):
        v = self.count == 1
        static = v & (self.src == STATIC)
        # an item of a static list belongs to workgroup (slot mod width) of its own XCD
        assert np.array_equal(self.block[static], (self.xcd + 8 * (self.slot % self.width))[static])
        if not self.queue:
            assert static[v].all()
            return
        # queue: exactly the flat indices below prefix x width are static; the others were claimed, by a workgroup whose src-th queue is this XCD's
        assert np.array_equal(static[v], (self.flat < self.prefix * self.width)[v])
        claimed = v & ~static
        assert (self.src[claimed] < 8).all()
        assert np.array_equal((self.block[claimed] + self.shift + self.src[claimed]) & 7, self.xcd[claimed])
        if self.shift:  # a workgroup's own XCD is its (8 - shift)-th queue: nothing of it before that, so its FIRST queue is always foreign
            own = claimed & ((self.block & 7) == self.xcd)
            assert (self.src[own] == 8 - self.shift).all()
            first = claimed & (self.src == 0)
            assert first.any() and ((self.block[first] & 7) != self.xcd[first]).all()


class _Batch:
    """an instance of (d, m), `nb` statements, and their proofs from the regenerating path: computed once per module, never changed"""

    def __init__(self, make_ctx, d, m, nb):
        import torch

        import c_lwe_snarks_amd as mf

        sys.path.insert(0, ROOT)
        import bench

        self.torch = torch
        self.nb = nb
        self.p = p = mf.Params(d=d, m=m)
        self.ctx = c = make_ctx(p)
        c.set_seed(SEED)
        inst = bench.build_instance(mf, c, torch, p, 7 * d + m)
        c.ssp_prepare(inst["d_ssp"])
        self.d_ssp = inst["d_ssp"]
        self.d_crs = c.setup(inst["d_ssp"], inst["alpha"], inst["beta"], inst["s"], inst["sk"], inst["err"])
        self.stmts = _statements(np.random.default_rng(d + nb), p, nb, inst["bits"])
        self.log = torch.zeros(LOG_WORDS, dtype=torch.int32, device=self.d_crs.device)
        c.set_batch_image(False)
        try:
            self.want = c.prove_batch(self.d_crs, self.d_ssp, *self.stmts).clone()
        finally:
            c.set_batch_image(True)

    def prove(self, mode, shift=0, prefix=DEFAULT[2]):
        """the proofs and the logged launches of one call in queue mode `mode`; the context is back at its defaults afterwards"""
        c = self.ctx
        self.log.zero_()
        c.set_mm_queue(mode, shift, prefix)
        c.set_mm_claim_log(self.log)
        try:
            got = c.prove_batch(self.d_crs, self.d_ssp, *self.stmts)
            self.torch.cuda.synchronize()
            descs = c.mm_claim_log_launches()
        finally:
            c.set_mm_claim_log(None)
            c.set_mm_queue(*DEFAULT)
        words = self.log.cpu().numpy().view(np.uint32)
        return got, [_Launch(d, words) for d in descs]

    def check(self, mode, shift=0, prefix=DEFAULT[2], launches=None):
        got, ls = self.prove(mode, shift, prefix)
        assert self.torch.equal(got, self.want)
        assert ls or self.nb == 70  # (persistent launches there were ...
        assert all(l.queue == mode for l in ls)  # ... and in the mode asked for)
        if launches is not None:
            assert sorted(l.coeff_bytes for l in ls) == launches
        for l in ls:
            l.check_exactly_once()
            l.check_owners()
        return ls


@pytest.fixture(scope="module")
def batches(gpu_ctx_factory):
    made = {}

    def get(d, m, nb):
        if (d, m, nb) not in made:
            made[d, m, nb] = _Batch(gpu_ctx_factory, d, m, nb)
        return made[d, m, nb]

    return get


@pytest.mark.parametrize("nb", [70, 100])
@pytest.mark.parametrize("d", [256, 512, 1024])
@pytest.mark.parametrize("pack", [True, False])
def test_queue_and_static_walk_give_the_regenerating_paths_bytes(batches, d, pack, nb):
    """70 and 100 statements (6 and 8 groups), items of 1, 2 and 4 stages, both partial-product forms: mode 1 and mode 0 against the same bytes; with mode 0 the owners are the
    static map's"""
    b = batches(d, 300, nb)
    b.ctx.set_mm_pack(pack)
    try:
        queued = b.check(1)
        static = b.check(0)
    finally:
        b.ctx.set_mm_pack(True)
    assert [(l.nblk, l.ngt, l.map) for l in queued] == [(l.nblk, l.ngt, l.map) for l in static]
    assert all(l.prefix * l.width < l.nchunks * l.per_chunk for l in queued)  # (something was left for the queues)
    assert nb == 70 or 4 in [l.coeff_bytes for l in queued]


@pytest.mark.parametrize("pack", [True, False])
def test_two_super_groups_and_the_merged_bw_launch(batches, pack):
    """300 statements: two super-groups, of 16 and of 4 groups (k_mmstream_p twice), and b_w of both as ONE k_mmstream_pb launch of one-byte columns over m = 341 rows"""
    b = batches(512, 341, 300)
    b.ctx.set_mm_pack(pack)
    try:
        ls = b.check(1, launches=[1, 4, 4])
        b.check(0, launches=[1, 4, 4])
    finally:
        b.ctx.set_mm_pack(True)
    assert sorted(l.ngt for l in ls if l.coeff_bytes == 4) == [4, 16]  # (255 + 45 statements: eight and two groups per region)


@pytest.mark.parametrize("nb", [70, 100])
@pytest.mark.parametrize("width", [16, 8])
def test_narrower_grids_draw_from_the_same_queues(batches, width, nb):
    """16 and 8 workgroups per XCD (the S / AS launch; b_w keeps every CU): any number of workgroups can draw from a queue"""
    b = batches(512, 300, nb)
    b.ctx.set_mm_width(width, False)
    try:
        ls = b.check(1)
        b.check(0)
    finally:
        b.ctx.set_mm_width(32, False)
    assert nb == 70 or width in [l.width for l in ls]


@pytest.mark.parametrize("nb", [70, 100])
def test_queue_over_chunks_and_slots(batches, nb):
    """d = 1024 in chunks of 256 rows: four chunks, the queue's index runs over (chunk, slot)"""
    b = batches(1024, 300, nb)
    b.ctx.set_mm_chunk_rows(256)
    try:
        ls = b.check(1)
        b.check(0)
    finally:
        b.ctx.set_mm_chunk_rows(0)
    assert nb == 70 or 4 in [l.nchunks for l in ls]


@pytest.mark.parametrize("prefix", [0, 1, 10**6])
def test_static_prefix_lengths(batches, prefix):
    """no static prefix (every item is claimed), one round, and a prefix longer than the list (clamped to it: every queue is exhausted from the start)"""
    b = batches(512, 300, 100)
    ls = b.check(1, prefix=prefix)
    for l in ls:
        rounds = l.nchunks * l.per_chunk // l.width
        assert l.prefix == min(prefix, rounds)


@pytest.mark.parametrize("shift", [1, 5])
def test_every_item_run_by_a_foreign_xcds_workgroup(batches, shift):
    """start_shift: the workgroups of XCD x begin in the queue of XCD x + shift and have no static prefix, so whatever a workgroup takes before its first queue ran dry is
    another XCD's item (check_owners: the items of a workgroup's own XCD all come from its (8 - shift)-th queue)"""
    b = batches(512, 300, 100)
    ls = b.check(1, shift=shift)
    assert all(l.shift == shift and l.prefix == 0 for l in ls)


def test_counters_are_rearmed_before_every_launch(batches):
    """the same call twice in one context, and a queue launch directly after a rendezvous launch (whose counters share the allocation): equal bytes, equal log totals"""
    b = batches(512, 300, 100)
    first = b.check(1)
    second = b.check(1)
    assert [int(l.count.sum()) for l in first] == [int(l.count.sum()) for l in second]
    b.ctx.set_mm_stream(1, True, 2, 16)
    try:
        got, ls = b.prove(1)  # (the rendezvous modes keep the static walk, whatever the queue mode)
        assert b.torch.equal(got, b.want) and ls and all(l.queue == 0 for l in ls)
        for l in ls:
            l.check_exactly_once()
            l.check_owners()
    finally:
        b.ctx.set_mm_stream(1, True, 0, 64)
    third = b.check(1)
    assert [int(l.count.sum()) for l in first] == [int(l.count.sum()) for l in third]


@pytest.mark.parametrize("ngl", [4, 8])
def test_two_launches_in_flight_have_counters_of_their_own(batches, ngl):
    """set_batch_launch(ngl, False): the S groups of a round are one launch on the caller's stream and the AS groups another on the side stream, with no event between
    them, so the second launch's memset is queued -- and runs -- while the first launch is still claiming.  Counters shared by the two would drop the second launch's
    last rounds (zeroed before the first has stopped adding to them) or rerun the first's (zeroed under it).  d = 2048, 248 statements = 8 groups per region: a launch of 8
    groups is 16 rounds of 8-stage items, some 0.4 ms, against the few microseconds between the two launches' starts; with 4 groups per launch (8 rounds, no static
    prefix left) the first launch claims from its first item on.  Bytes, and every item of every launch exactly once."""
    b = batches(2048, 300, 248)
    b.ctx.set_batch_launch(ngl, False)
    try:
        for _ in range(2):
            ls = b.check(1, launches=[4] * (16 // ngl))
        b.check(0, launches=[4] * (16 // ngl))
    finally:
        b.ctx.set_batch_launch(8, True)
    assert all(l.ngt == ngl for l in ls)
    assert (ngl == 8) == all(l.prefix > 0 for l in ls)
