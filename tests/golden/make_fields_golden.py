"""Generates tests/golden/fields.npz from the reference's OWN GaussianModel.extract_fields (gs_renderer.py:490-573), run unchanged
on the CPU in fp32. Like make_golden.py it runs only where the reference checkout is; nothing of the reference travels: the fixture
holds arrays. Per case <name>/: xyz, opacity, scaling, rotation (the raw leaves), resolution, num_blocks, relax_ratio, and the
reference's occ, center, scale. What the cases are for: tests/test_fields_gpu.py.

  basic     300 rows, 16^3, 4 blocks, relax 1.5
  cluster   700 rows, 600 of them inside one block, 18^3, 4 blocks: five chunks an axis, the last of 2 coordinates
  gaps      60 rows, 16^3, 4 blocks, relax 0: centres between chunks belong to no block, and some blocks are empty
  all       300 rows, 8^3, 1 block, relax 100: every row in the one block
  wide      200 rows, 24^3, 2 blocks: 1728 voxels a block
  filter    300 rows, 40 of them at logit -6 and far outside the others, 16^3, 4 blocks
  many      70 001 rows, 8^3, 2 blocks: row i is base row i % 257 moved by shift i // 257 (fields_ref.expand; the fixture holds
            the 257 base rows and the 273 shifts)
  stretch   300 rows, 16^3, 4 blocks, per-axis log-scale noise of sigma 0.8 (the others: 0.3)
Every case meets fields_ref.margins: no normalised centre within 1e-5 of a chunk gate and no opacity within 1e-6 of 0.005; a seed that does
not is replaced by the next one.
Usage: python tests/golden/make_fields_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository and the reference on sys.path)
from tests import fields_ref as FR  # noqa: E402  (the seeded inputs, shared with the tests)

MANY_BASE, MANY_ROWS = 257, 70001
draw, expand = FR.draw, FR.expand


def check(leaves, resolution, num_blocks, relax_ratio) -> bool:
    gate, opacity = FR.margins(leaves, resolution, num_blocks, relax_ratio)
    return gate >= FR.GATE_MARGIN and opacity >= FR.OPACITY_MARGIN


def cases():
    """name -> (leaves, resolution, num_blocks, relax_ratio, extra arrays)."""
    out = {}

    def add(name, seed, make, resolution, num_blocks, relax_ratio):
        while True:
            leaves, extra = make(np.random.default_rng(seed))
            full = expand(leaves, extra["shift"], MANY_ROWS) if "shift" in extra else leaves
            if check(full, resolution, num_blocks, relax_ratio):
                break
            seed += 1000
        out[name] = (leaves, full, resolution, num_blocks, relax_ratio, extra)

    add("basic", 1, lambda r: (draw(r, 300), {}), 16, 4, 1.5)

    def cluster(r):
        a, b = draw(r, 100), draw(r, 600, spread=0.06, size=0.03)
        b["xyz"] += np.float32([0.21, -0.17, 0.12])
        return {k: np.concatenate((a[k][:50], b[k], a[k][50:])) for k in a}, {}
    add("cluster", 2, cluster, 18, 4, 1.5)
    # wide enough that no value of a non-empty block underflows: its zeros are the empty blocks' and nothing else
    add("gaps", 3, lambda r: (draw(r, 60, size=0.1), {}), 16, 4, 0.0)
    add("all", 4, lambda r: (draw(r, 300), {}), 8, 1, 100.0)
    add("wide", 5, lambda r: (draw(r, 200), {}), 24, 2, 1.5)

    def filtered(r):
        d = draw(r, 300)
        low = r.choice(300, size=40, replace=False)
        d["opacity"][low] = -6.0
        d["xyz"][low] *= 10.0
        return d, {}
    add("filter", 6, filtered, 16, 4, 1.5)

    def many(r):
        d = draw(r, MANY_BASE, size=0.02)
        d["opacity"][::9] = -6.0
        shift = (r.uniform(-0.2, 0.2, size=(-(-MANY_ROWS // MANY_BASE), 3))).astype(np.float32)
        return d, {"shift": shift, "rows": np.int64(MANY_ROWS)}
    add("many", 7, many, 8, 2, 1.5)
    add("stretch", 8, lambda r: (draw(r, 300, sigma=0.8), {}), 16, 4, 1.5)
    return out


def main():
    MG.install_stubs()
    MG.cuda_to_cpu()
    import gs_renderer as G
    flat = {"cases": np.array(sorted(cases()))}
    for name, (leaves, full, resolution, num_blocks, relax_ratio, extra) in cases().items():
        gm = G.GaussianModel({"sh_degree": 0}, "scene")
        gm._xyz, gm._opacity = torch.tensor(full["xyz"]), torch.tensor(full["opacity"])
        gm._scaling, gm._rotation = torch.tensor(full["scaling"]), torch.tensor(full["rotation"])
        occ = gm.extract_fields(resolution, num_blocks, relax_ratio)
        rec = dict(leaves, **extra, resolution=np.int64(resolution), num_blocks=np.int64(num_blocks),
                   relax_ratio=np.float64(relax_ratio), occ=occ.numpy(), center=gm.center.numpy(), scale=np.float64(gm.scale))
        flat.update({f"{name}/{k}": np.asarray(v) for k, v in rec.items()})
        print(name, full["xyz"].shape[0], "rows", tuple(occ.shape), "max", float(occ.max()), "zeros", int((occ == 0).sum()),
              "least positive", float(occ[occ > 0].min()))
    path = os.path.join(HERE, "fields.npz")
    np.savez_compressed(path, **flat)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
