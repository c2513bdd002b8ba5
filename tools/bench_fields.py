"""Occupancy field extraction (GaussianModel.extract_fields, gs_renderer.py:490-573) two ways on the GPU:
  torch   the reference's op sequence as a torch chain (tests/fields_ref.py): a Python loop over num_blocks^3 blocks, one host
          synchronisation and a dozen pointwise kernels per block and 1024-Gaussian batch;
  fused   fields.extract_fields (csrc/fields.hip): five launches and one host read.
Shapes: 100 k rows at 64^3 in 8 blocks, 500 k rows at 128^3 in 16 blocks (synthetic object statistics, tests/fields_ref.draw).
Method (guide: measuring on the MI355X): one warm-up call and ONE timed call of the torch chain per shape, because it is slow; the
fused call is the median of five, each closed by a device synchronisation (it reads the bounds on the host anyway). Then the split
of the fused kernels, from device events around gsr_extract_fields alone: the full call against the same call with gates no centre
passes (every workgroup walks all membership words and evaluates nothing) -- scan against evaluation. Extraction is one-off work
per model: there is no pass bar.
usage: python tools/bench_fields.py [--shapes 100000:64:8,500000:128:16] [--no-torch] [--calls 5]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RELAX = 1.5


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def kernel_split(leaves, resolution, num_blocks, dev, calls):
    """ms of gsr_extract_fields (prepare + eval) by device events: as called, and with gates that admit no centre."""
    from dreamscene_amd import _lib as L
    from dreamscene_amd import fields as F
    lib = L.load()
    xyz, opacity, scaling, rotation = leaves
    P = xyz.shape[0]
    r = F.extract_fields(*leaves, resolution, num_blocks, RELAX)
    t = F.chunk_tables(resolution, num_blocks, RELAX)
    scratch = torch.empty(F.scratch_bytes(P), dtype=torch.uint8, device=dev)
    occ = torch.empty((resolution,) * 3, device=dev)
    center = (ctypes.c_float * 3)(*r.center.tolist())
    shut = torch.full_like(t.lo, float("inf"))
    out = {}
    for name, lo in (("full", t.lo), ("scan_only", shut)):
        table = torch.cat((t.coords, lo, t.hi)).to(dev)
        coords, glo, ghi = table.split((resolution, t.n_chunks, t.n_chunks))
        ms = []
        for _ in range(calls + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream = torch.cuda.current_stream(dev)
            a.record(stream)
            L.check(lib.gsr_extract_fields(xyz.data_ptr(), opacity.data_ptr(), scaling.data_ptr(), rotation.data_ptr(), P, center,
                                           r.scale, coords.data_ptr(), glo.data_ptr(), ghi.data_ptr(), resolution, t.split_size,
                                           t.n_chunks, occ.data_ptr(), scratch.data_ptr(), scratch.numel(), stream.cuda_stream),
                    "gsr_extract_fields")
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name + "_ms"] = round(statistics.median(ms[1:]), 4)
        if name == "scan_only":
            assert not bool(occ.any())
    out["scan_share"] = round(out["scan_only_ms"] / out["full_ms"], 4)
    n = t.n_chunks
    out["scan_bytes"] = n ** 3 * max(1, -(-t.split_size ** 3 // 1024)) * P * 8
    return out


def shape(P, resolution, num_blocks, dev, calls, with_torch):
    from dreamscene_amd import fields as F
    from tests import fields_ref as FR
    d = FR.draw(np.random.default_rng(P), P)
    leaves = [torch.tensor(d[k]).to(dev) for k in FR.LEAVES]
    fused = lambda: F.extract_fields(*leaves, resolution, num_blocks, RELAX)
    fused()
    times = [timed(fused, dev) for _ in range(calls)]
    got = times[-1][1]
    out = {"rows": P, "resolution": resolution, "num_blocks": num_blocks, "relax_ratio": RELAX, "kept": got.kept,
           "fused_ms": round(1e3 * statistics.median(t for t, _ in times), 4),
           "fused_calls_ms": [round(1e3 * t, 4) for t, _ in times]}
    out.update(kernel_split(leaves, resolution, num_blocks, dev, calls))
    if with_torch:
        chain = lambda: FR.extract_fields(*leaves, resolution, num_blocks, RELAX)
        FR.extract_fields(*[t[:2000] for t in leaves], resolution, num_blocks, RELAX)          # warm-up: the ops, not the shape
        seconds, (want, _, _, _) = timed(chain, dev)
        out["torch_ms"] = round(1e3 * seconds, 2)
        out["torch_over_fused"] = round(out["torch_ms"] / out["fused_ms"], 1)
        out["max_abs_diff_over_max"] = float((got.occ - want).abs().max() / want.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000:64:8,500000:128:16")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for s in a.shapes.split(","):
        P, resolution, num_blocks = (int(x) for x in s.split(":"))
        print(json.dumps({"tool": "bench_fields", **shape(P, resolution, num_blocks, dev, a.calls, not a.no_torch)}), flush=True)


if __name__ == "__main__":
    main()
