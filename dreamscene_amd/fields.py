"""Occupancy field extraction: `GaussianModel.extract_fields` of the reference (gs_renderer.py:490-573 with `gaussian_3d_coeff`,
:95-121) as two fused passes (csrc/fields.hip; SEMANTICS.md section 18).

  chunk_tables     the axis coordinates and the chunk gates, formed by torch on the host exactly as the reference forms them
  normalisation    center and scale from the bounds of the kept rows
  extract_fields   bounds (three launches, the one host read), then prepare and eval (two launches) -> FieldResult

The reference loops over num_blocks^3 blocks in Python, masks all Gaussians per block and launches a dozen pointwise kernels per
1024-Gaussian batch; here every chunk triple's workgroups walk the rows once and sum their members in index order. There is no
pair list and no capacity. No CPU fallback: tensors that are not on a ROCm device are refused with `GsrError`.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import _lib as L

MIN_OPACITY = 0.005                # a row is kept iff sigmoid(raw opacity) > MIN_OPACITY
EXTENT = 1.8                       # the kept rows' largest extent after normalisation
MAX_CHUNKS = 255                   # csrc/fields.hip: a chunk index is 8 bits of a row's membership word
MAX_RESOLUTION = 1024
HEAD_WORDS = 8                     # what gsr_fields_bounds writes at the start of the scratch: mn[3], mx[3], count, 0


class ChunkTables(NamedTuple):
    coords: torch.Tensor           # [resolution] fp32, host: torch.linspace(-1, 1, resolution)
    lo: torch.Tensor               # [n_chunks] fp32, host: a chunk's first coordinate - block_size * relax_ratio
    hi: torch.Tensor               # [n_chunks] fp32, host: its last coordinate + block_size * relax_ratio
    split_size: int
    n_chunks: int


class FieldResult(tuple):
    """(occ, center, scale, kept): fp32 [resolution]^3 and fp32 [3] on the device, a Python float, the number of kept rows."""
    occ = property(lambda self: self[0])
    center = property(lambda self: self[1])
    scale = property(lambda self: self[2])
    kept = property(lambda self: self[3])


def chunk_tables(resolution: int, num_blocks: int, relax_ratio: float) -> ChunkTables:
    """The reference's `linspace(-1, 1, resolution).split(resolution // num_blocks)` and, per chunk, its `vmin - block_size *
    relax_ratio` and `vmax + block_size * relax_ratio` in fp32. Raises ValueError where the reference asserts or cannot split."""
    block_size = 2 / num_blocks
    if resolution % block_size != 0:               # evaluated literally, as the reference's assert is
        raise ValueError(f"extract_fields: resolution {resolution} % block size {block_size} != 0")
    split_size = resolution // num_blocks
    if split_size < 1:
        raise ValueError(f"extract_fields: resolution {resolution} // num_blocks {num_blocks} < 1: nothing to split by")
    coords = torch.linspace(-1, 1, resolution)
    chunks = coords.split(split_size)
    if len(chunks) > MAX_CHUNKS or resolution > MAX_RESOLUTION:
        raise ValueError(f"extract_fields: {len(chunks)} chunks an axis at resolution {resolution}; at most {MAX_CHUNKS} chunks "
                         f"and a resolution of {MAX_RESOLUTION}")
    lo = torch.stack([c[0] for c in chunks])
    hi = torch.stack([c[-1] for c in chunks])
    lo -= block_size * relax_ratio
    hi += block_size * relax_ratio
    return ChunkTables(coords, lo, hi, split_size, len(chunks))


def normalisation(mn: torch.Tensor, mx: torch.Tensor, kept: int):
    """(center fp32 [3], scale float) from the kept rows' per-axis bounds: `(mn + mx) / 2` in fp32 and the Python division
    `1.8 / (mx - mn).amax().item()`. No kept row: ValueError; zero extent: ZeroDivisionError, as in the reference."""
    if kept <= 0:
        raise ValueError(f"extract_fields: no row has an opacity above {MIN_OPACITY}")
    center = (mn + mx) / 2
    scale = EXTENT / (mx - mn).amax().item()
    if not (math.isfinite(scale) and bool(torch.isfinite(center).all())):
        raise ValueError("extract_fields: the kept rows' bounds are not finite")
    return center, scale


def scratch_bytes(P: int) -> int:
    """Bytes of scratch a call on P rows needs (the `scratch=` of extract_fields)."""
    return int(L.load().gsr_fields_scratch_bytes(_rows(int(P))))


def _rows(P: int) -> int:
    if P <= 0:
        raise ValueError("extract_fields: no rows (P == 0)")
    if P > 2 ** 31 - 1:
        raise ValueError(f"extract_fields: {P} rows do not fit an int32")
    return P


def _leaf(t: torch.Tensor, shape, what: str, dev=None) -> torch.Tensor:
    t = t.detach()
    if t.device.type != "cuda":
        raise L.GsrError(f"fields.extract_fields needs its tensors on a cuda (ROCm) device, got {what} on {t.device}; there is no "
                         "CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"extract_fields: {what} must be fp32, got {t.dtype}")
    if dev is not None and t.device != dev:
        raise ValueError(f"extract_fields: {what} is on {t.device}, xyz on {dev}")
    if t.numel() != math.prod(shape):
        raise ValueError(f"extract_fields: {what} has {t.numel()} elements, not {shape}")
    return t.reshape(shape).contiguous()


@torch.no_grad()
def extract_fields(xyz: torch.Tensor, opacity_raw: torch.Tensor, scaling_raw: torch.Tensor, rotation_raw: torch.Tensor,
                   resolution: int = 128, num_blocks: int = 16, relax_ratio: float = 1.5, *, out: Optional[torch.Tensor] = None,
                   scratch: Optional[torch.Tensor] = None) -> FieldResult:
    """The raw leaves of a model (xyz [P,3], opacity logits [P,1], log-scales [P,3], quaternions [P,4]) -> FieldResult.
    out: an fp32 [resolution]^3 tensor to write instead of allocating one (every element is written). scratch: a uint8 tensor of
    scratch_bytes(P); its contents do not matter. The host waits once, for the bounds of the kept rows."""
    resolution, num_blocks = int(resolution), int(num_blocks)
    tables = chunk_tables(resolution, num_blocks, relax_ratio)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"extract_fields: xyz must be [P,3], got {tuple(xyz.shape)}")
    P = _rows(xyz.shape[0])
    xyz = _leaf(xyz, (P, 3), "xyz")
    dev = xyz.device
    opacity_raw = _leaf(opacity_raw, (P,), "opacity", dev)
    scaling_raw = _leaf(scaling_raw, (P, 3), "scaling", dev)
    rotation_raw = _leaf(rotation_raw, (P, 4), "rotation", dev)
    shape = (resolution,) * 3
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    elif out.device != dev or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"extract_fields: out must be a contiguous fp32 {shape} tensor on {dev}")
    lib = L.load()
    need = int(lib.gsr_fields_scratch_bytes(P))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif scratch.device != dev or scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < need:
        raise ValueError(f"extract_fields: scratch must be a contiguous uint8 tensor of at least {need} bytes on {dev}")
    head = torch.empty(HEAD_WORDS, dtype=torch.int32, pin_memory=True)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        L.check(lib.gsr_fields_bounds(xyz.data_ptr(), opacity_raw.data_ptr(), P, scratch.data_ptr(), scratch.numel(),
                                      stream.cuda_stream), "gsr_fields_bounds")
        torch.autograd.graph.increment_version(scratch)
        head.copy_(scratch[:4 * HEAD_WORDS].view(torch.int32), non_blocking=True)
        stream.synchronize()                       # the feature's one host read
        kept = int(head[6])
        bounds = head[:6].view(torch.float32)
        center, scale = normalisation(bounds[:3].clone(), bounds[3:].clone(), kept)
        table = torch.cat((tables.coords, tables.lo, tables.hi)).to(dev)
        coords, lo, hi = table.split((resolution, tables.n_chunks, tables.n_chunks))
        L.check(lib.gsr_extract_fields(xyz.data_ptr(), opacity_raw.data_ptr(), scaling_raw.data_ptr(), rotation_raw.data_ptr(), P,
                                       (C.c_float * 3)(*center.tolist()), scale, coords.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                       resolution, tables.split_size, tables.n_chunks, out.data_ptr(), scratch.data_ptr(),
                                       scratch.numel(), stream.cuda_stream), "gsr_extract_fields")
    torch.autograd.graph.increment_version(out)
    return FieldResult((out, center.to(dev), scale, kept))
