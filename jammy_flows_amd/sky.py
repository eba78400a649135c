"""Sky maps on the device (include/jammy_hip_sky.h, csrc/sky_kernels.hip): the HEALPix pixelisation of the sphere in the NESTED scheme and
adaptive multi-order meshes, batched over rows (conditional inputs) -- what the reference takes from healpy / mhealpy
(helper_fns/plotting/spherical.py:452-549).

Pixel ids: order o in [0, 29], nside = 2^o, 12 * 4^o pixels of equal area; the cells of a multi-order mesh carry NUNIQ ids
uniq = 4 * 4^o + pix, and uniq = -1 is padding.  The id and area arithmetic (uniq_of, order_pix_of, cell_log_area) is integer torch and works on
host tensors too; everything that touches directions or samples runs in the kernels and needs device tensors (there is no CPU path)."""
import math

import torch

from . import _hip

MAX_ORDER = _hip.SKY_MAX_ORDER
LOG_BASE_AREA = math.log(math.pi / 3.0)          # log of the area of an order-0 pixel, 4 pi / 12
LOG_4 = math.log(4.0)


def _check_order(order):
    if isinstance(order, bool) or not isinstance(order, int) or not 0 <= order <= MAX_ORDER:
        raise ValueError("order must be an integer in [0, %d], got %r" % (MAX_ORDER, order))


def uniq_of(order, pix):
    """NUNIQ ids of the pixels `pix` (int64 tensor) at `order` (an integer, or an int64 tensor of pix's shape); negative pixels give -1."""
    if isinstance(order, torch.Tensor):
        base = torch.bitwise_left_shift(torch.full_like(pix, 4), 2 * order.clamp(min=0))
    else:
        _check_order(order)
        base = 4 << (2 * order)
    return torch.where(pix >= 0, pix + base, torch.full_like(pix, -1))


def order_pix_of(uniq):
    """(order, pix) of NUNIQ ids, both int64 of uniq's shape; padding (ids below 4) gives (-1, -1).  Integer arithmetic only: five halving
    steps find floor(log4(uniq / 4))."""
    valid = uniq >= 4
    v = torch.where(valid, uniq, torch.full_like(uniq, 4)) >> 2          # in [4^o, 4 * 4^o)
    order = torch.zeros_like(uniq)
    for s in (16, 8, 4, 2, 1):
        hi = v >> (2 * s)
        take = hi > 0
        order = order + take.to(uniq.dtype) * s
        v = torch.where(take, hi, v)
    pix = uniq - torch.bitwise_left_shift(torch.full_like(uniq, 4), 2 * order)
    minus = torch.full_like(uniq, -1)
    return torch.where(valid, order, minus), torch.where(valid, pix, minus)


def cell_log_area(uniq):
    """log of the solid angle (steradian) of the cells, float64: log(pi / 3) - order * log 4; padding gives 0."""
    order, _ = order_pix_of(uniq)
    return torch.where(order >= 0, LOG_BASE_AREA - order.to(torch.float64) * LOG_4, torch.zeros((), dtype=torch.float64, device=uniq.device))


def cell_start(uniq):
    """first order-29 index of the cells' ranges [pix * 4^(29 - o), (pix + 1) * 4^(29 - o)); padding gives -1."""
    order, pix = order_pix_of(uniq)
    return torch.where(order >= 0, torch.bitwise_left_shift(pix, 2 * (MAX_ORDER - order).clamp(min=0)), pix)


def vec2pix(order, points, status=None):
    """NESTED pixel at `order` of directions: points (..., 3) vectors of any length or (..., 2) angles (zenith, azimuth), float32 or float64 on
    the device -> int64 (...,).  A non-finite row, a zero vector or a zenith outside [0, pi] gives -1 and is counted in `status`
    (_hip.new_status) under JF_STATUS_NONFINITE.  pix(order) == pix(29) >> 2 * (29 - order) exactly (jf_sky_vec2pix)."""
    _check_order(order)
    if points.dim() < 1 or points.shape[-1] not in (2, 3):
        raise ValueError("vec2pix: expected (..., 3) vectors or (..., 2) angles, got shape %s" % (tuple(points.shape),))
    suf = _hip._suffix(points)
    dev = _hip.require_device(points, status)
    _hip._sky()
    p = points.reshape(-1, points.shape[-1]).contiguous()
    out = torch.empty(p.shape[0], dtype=torch.int64, device=p.device)
    _hip._launch("jf_sky_vec2pix" + suf, "sky", (_hip._ptr(p), p.shape[1], p.shape[1], p.shape[0], order, _hip._ptr(out), _hip._ptr(status)), dev)
    return out.reshape(points.shape[:-1])


def cell_centres(uniq, vectors=True, dtype=torch.float64):
    """centres of the cells `uniq` (int64, any shape, on the device) -> (..., 3) unit vectors or, with vectors=False, (..., 2) angles (zenith,
    azimuth in [0, 2 pi)).  Padding gives the north pole (jf_sky_cell_centres)."""
    if uniq.dtype != torch.int64:
        raise ValueError("cell_centres: uniq must be int64, got %s" % uniq.dtype)
    dev = _hip.require_device(uniq)
    _hip._sky()
    ncol = 3 if vectors else 2
    u = uniq.reshape(-1).contiguous()
    out = torch.empty((u.shape[0], ncol), dtype=dtype, device=uniq.device)
    _hip._launch("jf_sky_cell_centres" + _hip._suffix(out), "sky", (_hip._ptr(u), u.shape[0], ncol, _hip._ptr(out), ncol), dev)
    return out.reshape(tuple(uniq.shape) + (ncol,))


def cell_counts(sorted_pix, uniq, row_of_cell):
    """counts (n,) int64: how many entries of row row_of_cell[i] of sorted_pix (G, S) -- order-29 indices, each row ascending -- fall into
    cell uniq[i] (jf_sky_cell_counts)."""
    dev = _hip.require_device(sorted_pix, uniq, row_of_cell)
    _hip._sky()
    if sorted_pix.dim() != 2 or sorted_pix.dtype != torch.int64 or uniq.dtype != torch.int64 or row_of_cell.dtype != torch.int64 \
            or uniq.dim() != 1 or uniq.shape != row_of_cell.shape:
        raise ValueError("cell_counts: expected int64 sorted_pix (G, S) and uniq, row_of_cell (n,)")
    sorted_pix, uniq, row_of_cell = sorted_pix.contiguous(), uniq.contiguous(), row_of_cell.contiguous()
    G, S = sorted_pix.shape
    counts = torch.empty_like(uniq)
    _hip._launch("jf_sky_cell_counts", "sky", (_hip._ptr(sorted_pix), S, G, S, _hip._ptr(uniq), _hip._ptr(row_of_cell), uniq.shape[0],
                                                _hip._ptr(counts)), dev)
    return counts


def locate(starts, offsets, pix):
    """index (G, T) int64 into `starts` of the leaf of row g that contains pix[g, t]: starts (total,) are the leaves' order-29 range starts,
    row g's in starts[offsets[g]:offsets[g + 1]], ascending; pix (G, T) order-29 indices.  -1 for a negative pixel (jf_sky_locate)."""
    dev = _hip.require_device(starts, offsets, pix)
    _hip._sky()
    if pix.dim() != 2 or offsets.dim() != 1 or offsets.shape[0] != pix.shape[0] + 1 or starts.dim() != 1 \
            or any(t.dtype != torch.int64 for t in (starts, offsets, pix)):
        raise ValueError("locate: expected int64 starts (total,), offsets (G + 1,) and pix (G, T)")
    # the kernel reads starts[offsets[g] .. offsets[g + 1]): the offsets are checked here, on the device, before it does
    if not bool((offsets[0] == 0) & (offsets[-1] == starts.shape[0]) & (offsets[1:] >= offsets[:-1]).all()):
        raise ValueError("locate: offsets must ascend from 0 to the number of cells (%d)" % starts.shape[0])
    starts, offsets, pix = starts.contiguous(), offsets.contiguous(), pix.contiguous()
    out = torch.empty_like(pix)
    _hip._launch("jf_sky_locate", "sky", (_hip._ptr(starts), _hip._ptr(offsets), pix.shape[0], _hip._ptr(pix), pix.shape[1], _hip._ptr(out)), dev)
    return out


def refine_select(lp, log_area, K, status=None):
    """the K most massive cells of every row -> sel (C, K) int64, ascending columns.  lp (C, M) log-densities (float32 or float64) and
    log_area float64 (M,), (C, M) or None, on the device; the key of a cell is (double)lp + log_area, the log of its probability mass.  The
    order is total -- a larger key wins, equal keys go to the lower column, NaN ranks as -inf and is counted in `status` under
    JF_STATUS_NONFINITE, -0.0 counts as +0.0 -- so the result is unique and a row's does not depend on the other rows
    (jf_sky_refine_select)."""
    return _hip.sky_refine_select(lp, log_area, K, status)


def refine_expand(uniq, lp, sel, status=None):
    """split the selected cells of every row into their four children -> (uniq_out (C, M + 3 K), lp_out (C, M + 3 K), new_cols (C, 4 K)).
    uniq (C, M) int64 NUNIQ ids in nested order, lp (C, M), sel (C, K) as refine_select returns it.  Cell m moves to column m + 3 * (number
    of selected columns below m); a selected cell's children 4 * uniq + j take its column and the three after it, lp_out is NaN there and
    new_cols names those columns, child by child.  The nested order of a row is preserved (jf_sky_refine_expand)."""
    return _hip.sky_refine_expand(uniq, lp, sel, status)


def map_entropy(lp, log_area, log_norm):
    """entropy (C,) float64 of the normalised piecewise-constant maps lp (C, M) with the cells' log_area (float64 (M,), (C, M) or None) and
    log_norm (C,) float64 = log sum exp(lp + log_area): log_norm - sum exp(lp + log_area - log_norm) * lp -- what the reference's
    s2_entropy_scanning sums over a flat map (jf_sky_refine_entropy)."""
    return _hip.sky_refine_entropy(lp, log_area, log_norm)


class Mesh:
    """C multi-order meshes in CSR form: row c's leaves are uniq[offsets[c]:offsets[c + 1]], ascending by their order-29 range start, and
    partition the sphere; counts holds the samples each leaf received."""

    def __init__(self, uniq, counts, offsets):
        self.uniq, self.counts, self.offsets = uniq, counts, offsets

    @property
    def rows(self):
        return self.offsets.shape[0] - 1

    def row_of_cell(self):
        sizes = self.offsets[1:] - self.offsets[:-1]
        return torch.repeat_interleave(torch.arange(self.rows, device=self.uniq.device), sizes, output_size=self.uniq.shape[0])

    def padded(self, values=None, fill=-1):
        """(C, Mmax) with row c's cells in its first columns: the ids (padding -1), or `values` (total,) laid out the same way (padding
        `fill`)"""
        values = self.uniq if values is None else values
        sizes = self.offsets[1:] - self.offsets[:-1]
        width = int(sizes.max()) if self.rows else 0
        row = self.row_of_cell()
        col = torch.arange(self.uniq.shape[0], device=self.uniq.device) - self.offsets[row]
        out = torch.full((self.rows, width), fill, dtype=values.dtype, device=values.device)
        out[row, col] = values
        return out

    def locate(self, pix29):
        """flat index (C, T) into uniq of the leaf of row c that holds each order-29 index of pix29 (C, T)"""
        return locate(cell_start(self.uniq), self.offsets, pix29)


def build_mesh(pix29, max_entries_per_cell=5, max_order=MAX_ORDER):
    """adaptive meshes of C sample sets, pix29 (C, S) order-29 indices on the device (vec2pix(29, ...); -1 entries are ignored) -> Mesh.

    The rule is moc_histogram's, as the reference uses it: starting from the 12 base pixels, a cell is split into its four children while
    it holds more than max_entries_per_cell samples and its order is below max_order; the leaves of one row are that row's mesh, which
    therefore depends on the row's own samples only.  Level by level for all rows at once: one sort of every row, then per level one
    jf_sky_cell_counts launch on the frontier of all rows and a compaction in torch -- one read-back (the frontier's size) per level."""
    _check_order(max_order)
    if pix29.dim() != 2 or pix29.dtype != torch.int64:
        raise ValueError("build_mesh: pix29 must be an int64 (C, S) tensor, got %s %s" % (pix29.dtype, tuple(pix29.shape)))
    if isinstance(max_entries_per_cell, bool) or not isinstance(max_entries_per_cell, int) or max_entries_per_cell < 0:
        raise ValueError("build_mesh: max_entries_per_cell must be a non-negative integer, got %r" % (max_entries_per_cell,))
    _hip.require_device(pix29)
    C = pix29.shape[0]
    dev = pix29.device
    sorted_pix = torch.sort(pix29, dim=1).values
    uniq = (torch.arange(12, device=dev) + 4).repeat(C)
    row = torch.arange(C, device=dev).repeat_interleave(12)
    child = torch.arange(4, device=dev)
    levels = []
    for order in range(max_order + 1):
        counts = cell_counts(sorted_pix, uniq, row)
        split = counts > max_entries_per_cell if order < max_order else torch.zeros_like(counts, dtype=torch.bool)
        levels.append((uniq, row, counts, ~split))
        if order == max_order:
            break
        idx = split.nonzero().reshape(-1)                  # (the read-back)
        if idx.shape[0] == 0:
            break
        uniq = (4 * uniq[idx, None] + child).reshape(-1)   # 4 * (4 * 4^o + p) + j = 4 * 4^(o + 1) + (4 p + j)
        row = row[idx].repeat_interleave(4)
    uniq, row, counts, leaf = (torch.cat(parts) for parts in zip(*levels))
    uniq, row, counts = uniq[leaf], row[leaf], counts[leaf]
    by_start = torch.argsort(cell_start(uniq))
    by_row = torch.sort(row[by_start], stable=True).indices
    perm = by_start[by_row]
    offsets = torch.zeros(C + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.bincount(row, minlength=C).cumsum(0)
    return Mesh(uniq[perm], counts[perm], offsets)
