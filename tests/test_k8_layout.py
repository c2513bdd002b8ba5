"""tests/k8_layout.py restates the workgroup layout of K8's sparse form (csrc/preprocess_bwd.hip: k8_plan, chunk_base). CPU: the
properties every user of it relies on."""
import numpy as np
import pytest

from tests import k8_layout as KL

SIZES = [1, 63, 64, 65, 2048, 2125, 262143, 262144, 262221, 500000]


@pytest.mark.parametrize("P", SIZES)
def test_blocks_partition_the_rows(P):
    rows, nb, nc = KL.sparse_layout(P)
    assert rows == (1024 if P >= 262144 else 256) and nb == -(-P // rows) and nc * 64 == rows
    seen = np.zeros(P, np.int32)
    for b in range(nb):
        r = KL.rows_of_block(P, b)
        assert r.size <= rows and (r >= 0).all() and (r < P).all()
        seen[r] += 1
        assert (KL.block_of_row(P, r) == b).all()
        # list order: chunk-major, then lane (ascending inside a chunk, chunks ascending)
        assert (np.diff(r) > 0).all()
        assert (np.diff(KL.chunk_of_row(P, r)) >= 0).all()
    assert (seen == 1).all()


@pytest.mark.parametrize("P", SIZES)
def test_chunks_past_the_end_are_empty_and_the_last_one_is_partial(P):
    rows, nb, nc = KL.sparse_layout(P)
    last_live = -1
    for b in range(nb):
        starts = KL.chunk_starts(P, b)
        assert starts.size == nc and (np.diff(starts) == nb * 64).all()
        r = KL.rows_of_block(P, b)
        per_chunk = np.bincount(KL.chunk_of_row(P, r), minlength=nc)
        for c, s in enumerate(starts):
            assert per_chunk[c] == max(0, min(64, P - int(s)))      # (0 for a chunk that starts at or past P)
            if s < P:
                last_live = max(last_live, int(s))
    assert last_live == (P - 1) // 64 * 64
    if P % 64:
        b = int(KL.block_of_row(P, [P - 1])[0])
        r = KL.rows_of_block(P, b)
        assert int((r >= last_live).sum()) == P % 64


@pytest.mark.parametrize("P", [2125, 262221])
def test_reach_counts(P):
    rng = np.random.default_rng(P)
    reached = rng.random(P) < 0.1
    cnt = KL.reach_counts(reached, P)
    _, nb, _ = KL.sparse_layout(P)
    assert cnt.shape == (nb,) and cnt.sum() == reached.sum()
    for b in (0, nb // 2, nb - 1):
        assert cnt[b] == reached[KL.rows_of_block(P, b)].sum()
