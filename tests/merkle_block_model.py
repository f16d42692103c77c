"""A brute-force model of a BLOCK -- transfers, adjusts and writes in any order -- on the records of an indexed table (words.Block, MerkleTree.apply_block /
apply_block_segments) for tests/test_merkle_block_cpu.py and tests/test_gpu_merkle_block.py: the table as a list of records, the tree of
tests/test_gpu_merkle.py's ref_tree over their hashlib digests, one step at a time on the table as it then stands.  A step's status is read off the records'
bytes; an applied step's new records are words.indexed_transfer's, indexed_adjust's or indexed_write's; its row is put together by the row builders of
tests/merkle_transfer_model.py, merkle_adjust_model.py and merkle_write_model.py."""
import numpy as np

import merkle_adjust_model as AM
import merkle_transfer_model as TM
import merkle_write_model as WM
from merkle_insert_model import InsertModel

NONE = 0xFFFFFFFF


def row_bytes(W, step, K, A, length, levels, cut=False):
    """the bytes of a step's row over `levels` levels; cut: a segment-0 row (a transfer's has 128 zero bytes in front)"""
    if step[0] == W.Block.TRANSFER:
        return TM.row_bytes(K, length, levels, A, 128 if cut else 64)
    if step[0] == W.Block.ADJUST:
        return AM.row_bytes(K, length, levels, A)
    return WM.row_bytes(K, length, levels, step[2][1] - step[2][0], step[4] is not None)


class BlockModel(InsertModel):
    """InsertModel (records, levels, set, siblings) with the steps of a words.Block"""

    def __init__(self, W, records, K, A=8):
        super().__init__(records, K)
        self.W, self.A = W, A

    def own(self, key):
        """the lowest live record whose own key is `key`, or None"""
        return next((i for i, r in enumerate(self.records) if self.live(i) and r[: self.K] == key), None)

    def balance(self, i):
        return int.from_bytes(self.records[i][2 * self.K: 2 * self.K + self.A], "big")

    def supply(self):
        return AM.supply(self.records, self.K, self.A)

    def status(self, step):
        """0 fine; 1 the key (a transfer's sender) is no member, 2 a transfer's receiver is none, 3 an overdraft, 4 an overflow, 5 the field is not what the
        step expects: the first that applies, on the table as it stands"""
        B, top = self.W.Block, 1 << (8 * self.A)
        i = self.own(step[1])
        if i is None:
            return 1
        if step[0] == B.TRANSFER:
            s = self.own(step[2])
            if s is None:
                return 2
            return 3 if step[3] > self.balance(i) else 4 if self.balance(s) + step[3] >= top else 0
        if step[0] == B.ADJUST:
            return 3 if step[3] and step[2] > self.balance(i) else 4 if not step[3] and self.balance(i) + step[2] >= top else 0
        lo, hi = step[2]
        return 5 if step[4] is not None and self.records[i][lo:hi] != step[4] else 0

    def slots(self, step):
        a = self.own(step[1])
        b = self.own(step[2]) if step[0] == self.W.Block.TRANSFER else None
        return (NONE if a is None else a, NONE if b is None else b)

    def updates(self, step):
        """[(slot, new record)] of an applied step on the table as it stands: what words.indexed_* say"""
        W, B, K, A = self.W, self.W.Block, self.K, self.A
        i = self.own(step[1])
        if step[0] == B.TRANSFER:
            s = self.own(step[2])
            idx, new = W.indexed_transfer(self.records[i], i, self.records[s], s, step[3], K, A)
            return [(idx[0], new[0].tobytes()), (idx[1], new[1].tobytes())]
        if step[0] == B.ADJUST:
            return [(i, W.indexed_adjust(self.records[i], step[2], step[3], K, A).tobytes())]
        return [(i, W.indexed_write(self.records[i], step[2], step[3], K, expect=step[4]).tobytes())]

    def apply(self, block, skip_failed=True, cuts=None):
        """the steps in order, a step with a status left out.  A dict: index [nk, 2], status [nk], rows (a packed row per step, None for a skipped one; with
        cuts the segment-0 rows), roots [nk + 1, 32], first_update [nk + 1], update_roots [nupd + 1, 32] and, with cuts, segments (one array [nupd, bytes] per
        upper level range) and nodes [nupd, G + 1, 2, 32].  skip_failed=False with a failed step: nothing is applied, rows are all None"""
        from merkle_segments_model import pack
        from merkle_segments_model import stand_in as any_stand_in

        W, B, K, A, depth, length = self.W, self.W.Block, self.K, self.A, self.depth, self.length
        judge = BlockModel(W, self.records, K, A)
        index, status = [], []
        for step in block.steps:
            index.append(judge.slots(step))
            status.append(judge.status(step))
            if not status[-1]:
                for i, rec in judge.updates(step):
                    judge.records[i] = rec  # (the tree is not needed here)
        out = {"index": np.array(index, dtype=np.uint32).reshape(len(block), 2), "status": np.array(status, dtype=np.uint8)}
        applied = [not s for s in status] if skip_failed or not any(status) else [False] * len(block)
        ranges = W.segment_levels(depth, cuts) if cuts else [(0, depth)]
        c0 = ranges[0][1]
        low = (1 << c0) - 1
        rows, roots, first, uroots = [], [self.root()], [0], [self.root()]
        segments, nodes = [[] for _ in ranges[1:]], []
        for step, go in zip(block.steps, applied):
            if not go:
                rows.append(None)
                roots.append(self.root())
                first.append(first[-1])
                continue
            olds, sibs = [], []
            if step[0] == B.TRANSFER:  # s's record is read AFTER p's update (p != s: the same bytes either way, but its siblings are not)
                p, s = self.own(step[1]), self.own(step[2])
                (_, new_p), (_, new_s) = self.updates(step)
                ups = [(p, new_p), (s, new_s)]
            else:
                ups = self.updates(step)
            for i, rec in ups:
                old_path = [self.levels[l][i >> l] for l in range(depth + 1)]
                olds.append(self.records[i])
                sibs.append(self.siblings(i))
                self.set(i, rec)
                new_path = [self.levels[l][i >> l] for l in range(depth + 1)]
                for g, (lo, hi) in enumerate(ranges[1:]):
                    st = any_stand_in(W.MerkleSegment, levels=hi - lo, depth=hi - lo)
                    segments[g].append(pack(st.bits(old_path[lo], new_path[lo], sibs[-1][lo:hi], (i >> lo) & ((1 << (hi - lo)) - 1))))
                nodes.append([[list(old_path[c]), list(new_path[c])] for c in [hi for _, hi in ranges]])
                uroots.append(self.root())
            if step[0] == B.TRANSFER:
                st0 = TM.stand_in(K, length, c0, A, joined=not cuts)
                (p, _), (s, _) = ups
                rows.append(pack(st0.bits(step[1], step[2], step[3], olds[0], olds[1], sibs[0][:c0], p & low, sibs[1][:c0], s & low)))
            elif step[0] == B.ADJUST:
                rows.append(AM.packed_row(step[1], step[2], step[3], olds[0], sibs[0][:c0], ups[0][0] & low, A))
            else:
                rows.append(WM.packed_row(step[1], step[4], step[3], olds[0], sibs[0][:c0], ups[0][0] & low))
            roots.append(self.root())
            first.append(first[-1] + len(ups))
        out.update(rows=rows, roots=np.array([list(r) for r in roots], dtype=np.uint8), first_update=np.array(first, dtype=np.uint32),
                   update_roots=np.array([list(r) for r in uroots], dtype=np.uint8))
        if cuts:
            out.update(segments=[np.array(s, dtype=np.uint8).reshape(len(nodes), -1) for s in segments], nodes=np.array(nodes, dtype=np.uint8).reshape(len(nodes), len(ranges), 2, 32))
        return out
