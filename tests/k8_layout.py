"""Which workgroup of K8's sparse form owns which Gaussian -- the layout of csrc/preprocess_bwd.hip (k8_plan picks the block
size, chunk_base places the chunks), restated ONCE for the tests that assert what a workgroup receives. Host only, numpy only.

  rows_per_block = 1024 from P = 262 144 on (KPER = 4), 256 below (KPER = 1)
  n_blocks       = ceil(P / rows_per_block)
  chunk c of block b (c = 0 .. rows_per_block / 64 - 1) = the 64 rows from (c * n_blocks + b) * 64

so a block's chunks lie n_blocks * 64 rows apart, chunks that start at or past P are empty and the chunk that straddles P is
partial. The kernel lists a block's reached rows chunk-major, then by lane: rows_of_block returns that order, and entry e of the
reached rows of a block is handled in round e // 256 by wave slot (e % 256) // 64, which is wave (slot + b) % 4."""
import numpy as np

BIG_P = 262144          # k8_plan: 256 * kK8Block
CHUNK = 64


def sparse_layout(P):
    """-> (rows_per_block, n_blocks, chunks_per_block)"""
    P = int(P)
    rows = 1024 if P >= BIG_P else 256
    return rows, (P + rows - 1) // rows, rows // CHUNK


def chunk_starts(P, b):
    """first row of every chunk of block b (those at or past P included: they are empty)"""
    _, nb, nc = sparse_layout(P)
    return (np.arange(nc, dtype=np.int64) * nb + int(b)) * CHUNK


def rows_of_block(P, b):
    """the rows block b owns, in the kernel's list order: chunk-major, then lane"""
    r = (chunk_starts(P, b)[:, None] + np.arange(CHUNK, dtype=np.int64)[None, :]).reshape(-1)
    return r[r < int(P)]


def block_of_row(P, rows):
    _, nb, _ = sparse_layout(P)
    return (np.asarray(rows, dtype=np.int64) // CHUNK) % nb


def chunk_of_row(P, rows):
    _, nb, _ = sparse_layout(P)
    return (np.asarray(rows, dtype=np.int64) // CHUNK) // nb


def reach_counts(reached, P):
    """reached: bool [P] -> reached rows per block, int64 [n_blocks]"""
    reached = np.asarray(reached, dtype=bool).reshape(-1)
    assert reached.size == int(P)
    _, nb, _ = sparse_layout(P)
    return np.bincount(block_of_row(P, np.nonzero(reached)[0]), minlength=nb).astype(np.int64)
