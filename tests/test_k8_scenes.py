"""CPU, oracle only: the scenes of tests/k8_scenes.py deliver, per workgroup of K8's sparse form, what tests/test_k8_blocks.py
relies on. Everything is asserted from the C oracle's outputs (radii, the rows its forward blended, the rows its backward gave a
gradient), never from the recipe. Prints the per-block reached counts and the two pair counts per scene (pytest -s)."""
import numpy as np
import pytest

from tests import k8_layout as KL
from tests import k8_scenes as KS

V = 4
SCENES = [(2125, 0), (2125, 1), (262221, 0), (262143, 1)]      # (262 143: the last P that takes 256-row blocks, 1 024 of them)


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    yield
    KS.forget()      # (the cached cases hold about 200 MB of host memory each at the big sizes)


@pytest.mark.parametrize("P,seed", SCENES)
def test_blocks_receive_the_planned_lists(c_oracle, P, seed):
    case = KS.oracle_case(c_oracle, P, 16, 3, V, seed)
    des, reached, views = case["des"], case["reached"], case["views"]
    union = reached.any(0)
    blended = np.stack([v["blended"] for v in views])
    radii = np.stack([v["radii"] for v in views])
    # the backward's rows = the rows the forward blended, view by view; over the views: the designated rows some view blends
    assert np.array_equal(reached, blended)
    assert np.array_equal(union, des & blended.any(0))
    assert not (union & ~des).any()
    counts = KL.reach_counts(union, P)
    plan = KS.plan_blocks(P, seed)
    print(f"\n[k8 scene P {P} seed {seed}] reached {int(union.sum())} of {int(des.sum())} designated; min final_T "
          f"{[round(v['min_T'], 5) for v in views]}")
    print(f"[k8 scene P {P} seed {seed}] reached rows per block: {counts.tolist()}")
    for b, name in sorted(plan.items()):
        print(f"[k8 scene P {P} seed {seed}] block {b:3d} {name:10s} {int(counts[b])}")
        assert counts[b] == KS.expected_count(P, b, name), (b, name)
    rows, nb, nc = KL.sparse_layout(P)
    names = set(plan.values())
    need = {"zero", "one", "slot0", "full", "sprinkle"} | ({"n255", "slot1", "slot2", "slot3", "last_chunk", "tail"} if nb >= 80
                                                          else set()) | ({"n256", "n257"} if rows == 1024 else set())
    assert need <= names, need - names
    for b, name in plan.items():
        if name.startswith("slot"):
            assert b % 4 == int(name[4])       # (the block rotation hands list slot 0 to wave b % 4)
            r = KL.rows_of_block(P, b)
            assert len(set(KL.chunk_of_row(P, r[union[r]]).tolist())) == 1      # one chunk: list entries 0..63, one wave slot
    # row P - 1 and the whole final partial chunk
    assert P % 64 and union[(P - 1) // 64 * 64:].all()
    # random extras: blocks outside the plan hold some rows and idle waves beside busy ones
    free = [b for b in range(nb) if b not in plan]
    if free:
        assert all(counts[b] < rows for b in free) and sum(0 < counts[b] <= rows - 64 for b in free) >= min(len(free), 32)
        assert sum(int(counts[b]) for b in free) >= 100
    # (row, view) pairs the kernel sees but does not take, and pairs it does not see, on rows another view reached
    seen_not_taken = (radii > 0) & ~reached & union[None]
    unseen = (radii == 0) & union[None]
    n1, n2 = int(seen_not_taken.sum()), int(unseen.sum())
    print(f"[k8 scene P {P} seed {seed}] pairs seen but not reached (row reached elsewhere): {n1}; pairs with radii == 0: {n2}")
    assert n1 >= 32 and n2 >= 32
    # every view matters: rows reached by the first view alone, and by the last view alone
    alone = [int((reached[j] & ~np.delete(reached, j, 0).any(0)).sum()) for j in range(V)]
    print(f"[k8 scene P {P} seed {seed}] rows reached by one view alone, per view: {alone}")
    assert alone[0] >= 8 and alone[-1] >= 8
    # seen-only rows (wave_exit's statistics): visible somewhere, reached nowhere
    assert int(((radii > 0).any(0) & ~union).sum()) >= 32
    # the layout's edges are in play: a block with a trailing chunk at or past P, and a block whose last live chunk is partial
    trailing = [b for b in range(nb) if (KL.chunk_starts(P, b)[1:] >= P).any()]
    partial = [b for b in range(nb) if KL.rows_of_block(P, b).size % 64]
    assert partial and all(counts[b] > 0 for b in partial)
    if nb * rows - P >= 64:       # (P = 262 143 fills every chunk of its 1 024 blocks but the last row)
        assert trailing and any(counts[b] > 0 for b in trailing)


def test_no_block_past_64_rows_has_only_its_first_chunk():
    """Chunk 1 of block b starts at (n_blocks + b) * 64 < P whenever P > 64 (n_blocks * 64 <= P / 4 + 64): "every chunk past
    the first lies at or beyond P" happens for P <= 64 only, where the one block has one live chunk."""
    for P in (40, 64):
        assert (KL.chunk_starts(P, 0)[1:] >= P).all() and KL.sparse_layout(P)[1] == 1
    for P in (65, 2125, 262143, 262144, 262221):
        _, nb, _ = KL.sparse_layout(P)
        assert all((KL.chunk_starts(P, b)[1] < P) for b in range(nb))
