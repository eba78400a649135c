"""GPU tests (run with -m gpu) of the density-refined sky maps: the selection, expansion and entropy kernels (csrc/sky_refine_kernels.hip
through sky.refine_select / refine_expand / map_entropy) and pdf.sky_map_adaptive.  Expected values never come from the code under test: a
numpy lexsort for the selection, Python integer arithmetic for the ids, numpy float64 sums on the device's own tile, a replay of the
refinement with numpy selection on the host, and the oracle."""
import math

import numpy as np
import pytest
import torch

import fixture_io
from helpers import build_oracle, build_product, to_dev
from test_gpu_sky import SKY_QS, check_row, oracle_block_logp, recompute, same_bits

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
NP = {F64: np.float64, F32: np.float32}
CHUNK = 256                                                  # columns per step of a row's walk
INF = float("inf")
LOG_BASE_AREA, LOG_4 = math.log(math.pi / 3.0), math.log(4.0)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------- select
def np_select(lp, logw, K):
    """the rule in numpy: key = (double)lp + logw in one addition, NaN as -inf, -0.0 as +0.0; larger key first, equal keys to the lower
    column; the K winners in ascending column order"""
    key = lp.astype(np.float64)
    if logw is not None:
        key = key + (logw if logw.ndim == 2 else logw[None])
    key = np.where(np.isnan(key), -INF, key)
    cols = np.arange(lp.shape[1])
    return np.stack([np.sort(np.lexsort((cols, -(k + 0.0)))[:K]) for k in key]).reshape(lp.shape[0], K)


def select_rows(M, np_dtype, seed):
    """three rows and their log-areas: (0) values from a small dyadic set, so that every rank falls into a run of equal keys, with dyadic
    log-areas, so that equal keys are made from different lp + logw and a coarser cell of lower density wins by its column; (1) continuous
    values with a run of -inf, +0.0 and -0.0 keys, a +inf and one NaN; (2) all equal"""
    rng = np.random.default_rng(seed)
    lp = np.empty((3, M))
    logw = np.empty((3, M))
    lp[0] = rng.integers(-4, 5, M) * 0.5
    logw[0] = rng.integers(0, 3, M) * -1.5
    lp[1] = rng.normal(size=M) * 3
    logw[1] = rng.integers(0, 4, M) * -LOG_4
    n_nan = 0
    if M >= 16:
        lp[1, 2:6] = -INF
        lp[1, 7], logw[1, 7] = 0.0, -0.0
        lp[1, 8], logw[1, 8] = -0.0, -0.0
        lp[1, 10], logw[1, 10] = -0.0, 0.0
        lp[1, 9] = INF
        lp[1, 12] = np.nan
        n_nan = 1
    elif M >= 4:
        lp[1, 0] = -INF
        lp[1, 1], logw[1, 1] = -0.0, -0.0
        lp[1, 2], logw[1, 2] = 0.0, 0.0
        lp[1, 3] = np.nan
        n_nan = 1
    lp[2] = -1.25
    logw[2] = LOG_BASE_AREA
    return lp.astype(np_dtype), logw, n_nan


@pytest.mark.parametrize("mode", ["rows", "shared", "none"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 255, 256, 257, 511, 513, 4095, 4097])
def test_select_vs_lexsort(M, dtype, mode):
    from jammy_flows_amd import _hip, sky
    lp, logw, n_nan = select_rows(M, NP[dtype], M)
    if mode == "shared":
        logw = logw[1]                                       # (row 1's: the signed zeros stay where its planted keys need them)
    elif mode == "none":
        logw = None
    d_lp, d_logw = dev(lp), None if logw is None else dev(logw)
    for K in sorted({0, 1, M // 4, M}):
        want = np_select(lp, logw, K)
        status = _hip.new_status("cuda")
        got = sky.refine_select(d_lp, d_logw, K, status)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, K)
        assert np.array_equal(host(got), want), (M, K, mode)
        assert status.tolist() == [0, n_nan if K > 0 else 0, 0, 0]
        for c in range(3):                                   # C = 1: a row launched alone gives the same columns
            w = d_logw if d_logw is None or d_logw.dim() == 1 else d_logw[c:c + 1]
            assert torch.equal(sky.refine_select(d_lp[c:c + 1], w, K), got[c:c + 1]), (M, K, mode, c)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_select_every_rank_of_rows_with_ties_zeros_and_infinities(dtype):
    """every K from 0 to M on short rows: the boundary passes through every run of equal keys, between -0.0 and +0.0, and past the -inf
    cells and the NaN"""
    from jammy_flows_amd import sky
    rows = np.array([[-0.0, 0.0, -0.0, 0.0, -1.0, INF, -INF, np.nan, -INF, 2.5, 2.5, INF, 0.0, -0.0],
                     [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                     [-INF, -INF, np.nan, -INF, -INF, -INF, np.nan, -INF, -INF, -INF, -INF, -INF, -INF, -INF]]).astype(NP[dtype])
    # equal keys from different summands: 2 - 1.5 == 1.5 - 1 == 0.5 + 0, and a lower density that wins on its area
    logw = np.array([[0.0, -0.0, 0.0, -0.0, 1.0, 0.0, 5.0, 0.0, -INF, -1.5, -1.0, -3.0, -0.0, 0.0],
                     [0.0, -1.5, 0.0, -1.5, 0.5, -1.5, 0.0, 0.5, 0.0, 0.0, -1.5, 0.5, 0.0, 0.0],
                     [0.0] * 14])
    M = rows.shape[1]
    for K in range(M + 1):
        for lw in (logw, logw[0], None):
            want = np_select(rows, lw, K)
            got = sky.refine_select(dev(rows), None if lw is None else dev(lw), K)
            assert np.array_equal(host(got), want), (K, lw is None or lw.ndim)
    # a long row of one value plus one larger cell at its end: the K winners are that cell and the first K - 1 columns
    M = 3 * CHUNK + 5
    row = np.full((1, M), -2.0, dtype=NP[dtype])
    row[0, -1] = -1.0
    for K in (1, 2, CHUNK, CHUNK + 1, M - 1):
        assert host(sky.refine_select(dev(row), None, K))[0].tolist() == list(range(K - 1)) + [M - 1]


# ---------------------------------------------------------------------------------------------- expand
def order_of(u):
    return (u.bit_length() - 3) // 2


def start_of(u):
    o = order_of(u)
    return (u - 4 * 4 ** o) * 4 ** (29 - o)


def nested_row(rng, n_splits, max_order=29):
    """a multi-order row that partitions the sphere, in nested order: the 12 base cells, n_splits times one random cell replaced by its
    children (Python integers)"""
    row = list(range(4, 16))
    for _ in range(n_splits):
        i = int(rng.integers(len(row)))
        if order_of(row[i]) < max_order:
            row[i:i + 1] = [4 * row[i] + j for j in range(4)]
    return row


def py_expand(uniq, lp, sel):
    """one row in Python: ids, values (None = a new child) and the new columns"""
    ids, vals, new_cols = [], [], []
    chosen = set(sel)
    for m, (u, v) in enumerate(zip(uniq, lp)):
        if m in chosen:
            new_cols += list(range(len(ids), len(ids) + 4))
            ids += [4 * u + j for j in range(4)]
            vals += [None] * 4
        else:
            ids.append(u)
            vals.append(v)
    return ids, vals, new_cols


def check_partition(ids):
    starts = [start_of(u) for u in ids]
    assert all(a < b for a, b in zip(starts, starts[1:]))
    assert sum(4 ** (29 - order_of(u)) for u in ids) == 12 * 4 ** 29


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_expand_vs_python(dtype):
    from jammy_flows_amd import _hip, sky
    rng = np.random.default_rng(5)
    C, n_splits = 3, 100
    M = 12 + 3 * n_splits                                    # 312 cells: two workgroups per row, rows that start inside a workgroup
    rows = [nested_row(rng, n_splits) for _ in range(C)]
    assert all(len(r) == M for r in rows)
    uniq = np.array(rows, dtype=np.int64)
    lp = rng.normal(size=(C, M)).astype(NP[dtype])
    lp[0, 3], lp[1, 0], lp[2, M - 1] = -INF, np.nan, INF     # kept values travel by their bits
    d_uniq, d_lp = dev(uniq), dev(lp)
    for K in (0, 1, 77, M):
        sel = np.stack([np.sort(rng.choice(M, K, replace=False)) for _ in range(C)]).reshape(C, K).astype(np.int64)
        status = _hip.new_status("cuda")
        uo, lo, nc = sky.refine_expand(d_uniq, d_lp, dev(sel), status)
        assert uo.dtype == torch.int64 and lo.dtype == dtype and nc.dtype == torch.int64
        assert tuple(uo.shape) == tuple(lo.shape) == (C, M + 3 * K) and tuple(nc.shape) == (C, 4 * K) and status.tolist() == [0, 0, 0, 0]
        for c in range(C):
            ids, vals, new_cols = py_expand(rows[c], lp[c], sel[c].tolist())
            assert host(uo)[c].tolist() == ids and host(nc)[c].tolist() == new_cols, (K, c)
            got = host(lo)[c]
            kept = [i for i, v in enumerate(vals) if v is not None]
            assert np.isnan(got[new_cols]).all() and len(kept) + len(new_cols) == M + 3 * K
            assert np.array_equal(got[kept].view(np.uint8), np.array([vals[i] for i in kept], dtype=NP[dtype]).view(np.uint8)), (K, c)
            check_partition(ids)
            assert host(sky.cell_start(uo[c])).tolist() == [start_of(u) for u in ids]
        if K == 0:
            assert torch.equal(uo, d_uniq) and same_bits(lo, d_lp)


def test_expand_of_a_full_map_is_the_next_order():
    from jammy_flows_amd import sky
    o = 2
    M = 12 * 4 ** o
    uniq = sky.uniq_of(o, torch.arange(M, device="cuda"))[None].repeat(2, 1)
    lp = torch.zeros((2, M), dtype=F64, device="cuda")
    sel = torch.arange(M, device="cuda")[None].repeat(2, 1)
    uo, lo, nc = sky.refine_expand(uniq, lp, sel)
    want = torch.arange(12 * 4 ** (o + 1), device="cuda") + 4 * 4 ** (o + 1)
    assert torch.equal(uo[0], want) and torch.equal(uo[1], want) and torch.equal(nc[1], torch.arange(4 * M, device="cuda"))
    assert bool(lo.isnan().all())


def test_expand_of_order_28_cells_and_a_cell_that_cannot_be_split():
    """ids near 2^60: the last pixel of order 28 has the children 2^62 - 4 .. 2^62 - 1.  A selected cell of order 29, or padding, stays, is
    followed by three padding cells and is counted"""
    from jammy_flows_amd import _hip, sky
    n28 = 12 * 4 ** 28
    row = [4 * 4 ** 28 + p for p in (0, 1, 4 ** 28 - 1, 4 ** 28, n28 - 2, n28 - 1)]
    uniq = dev(np.array([row], dtype=np.int64))
    lp = dev(np.arange(6, dtype=np.float64)[None])
    sel = dev(np.array([[0, 2, 5]], dtype=np.int64))
    status = _hip.new_status("cuda")
    uo, lo, nc = sky.refine_expand(uniq, lp, sel, status)
    ids, vals, new_cols = py_expand(row, list(range(6)), [0, 2, 5])
    assert ids[-1] == 2 ** 62 - 1 and host(uo)[0].tolist() == ids and host(nc)[0].tolist() == new_cols and status.tolist() == [0, 0, 0, 0]
    assert all(order_of(ids[i]) == 29 for i in new_cols)
    assert host(sky.order_pix_of(uo)[0])[0].tolist() == [order_of(u) for u in ids]
    assert host(sky.cell_start(uo))[0].tolist() == [start_of(u) for u in ids]
    # the children are of order 29 now; with a padding cell
    stuck = dev(np.array([[ids[0], ids[4], -1, ids[5]]], dtype=np.int64))
    assert order_of(ids[0]) == 29 and order_of(ids[4]) == 28
    lp = dev(np.array([[0.5, 1.5, 2.5, 3.5]]))
    uo, lo, nc = sky.refine_expand(stuck, lp, dev(np.array([[0, 1, 2]], dtype=np.int64)), status)
    assert host(uo)[0].tolist() == [ids[0], -1, -1, -1] + [4 * ids[4] + j for j in range(4)] + [-1, -1, -1, -1] + [ids[5]]
    assert host(nc)[0].tolist() == [-1] * 4 + [4, 5, 6, 7] + [-1] * 4
    got = host(lo)[0]
    assert got[[0, 8, 12]].tolist() == [0.5, 2.5, 3.5] and (got[[1, 2, 3, 9, 10, 11]] == -INF).all() and np.isnan(got[4:8]).all()
    assert status.tolist() == [0, 0, 2, 0]


def test_expand_counts_a_selection_that_breaks_its_contract():
    """entries outside [0, M), repeated or descending are counted under JF_STATUS_OUT_OF_RANGE, one per entry; a valid row beside them is
    expanded as always"""
    from jammy_flows_amd import _hip, sky
    M = 12
    uniq = dev(np.array([list(range(4, 16))] * 4, dtype=np.int64))
    lp = dev(np.arange(4 * M, dtype=np.float64).reshape(4, M))
    sel = dev(np.array([[1, 5, 9], [3, 3, 7], [8, 2, 11], [-1, 4, 12]], dtype=np.int64))       # fine; a repeat; descending; outside twice
    status = _hip.new_status("cuda")
    uo, lo, nc = sky.refine_expand(uniq, lp, sel, status)
    assert status.tolist() == [0, 0, 4, 0]
    ids, vals, new_cols = py_expand(list(range(4, 16)), list(range(M)), [1, 5, 9])
    assert host(uo)[0].tolist() == ids and host(nc)[0].tolist() == new_cols
    assert tuple(uo.shape) == (4, M + 9) and tuple(nc.shape) == (4, 12)


# ---------------------------------------------------------------------------------------------- entropy
def np_entropy(lp, log_area, ln):
    lp = lp.astype(np.float64)
    keep = lp != -INF
    a = lp[keep] + (0.0 if log_area is None else log_area[keep])
    return ln - (np.exp(a - ln) * lp[keep]).sum()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 255, 257, 4097])
def test_entropy_vs_numpy(M, dtype):
    """numpy float64 on the device's own tile, to M 2^-52 relative (the bar of the sums of test_gpu_sky.check_row)"""
    from jammy_flows_amd import sky
    rng = np.random.default_rng(M)
    C = 3
    lp = (rng.normal(size=(C, M)) * 3).astype(NP[dtype])
    if M > 8:
        lp[0, 1:5] = -INF
        lp[2, M - 1] = -INF
    log_area = LOG_BASE_AREA - rng.integers(0, 6, (C, M)) * LOG_4
    for la in (log_area, log_area[0], None):
        a = lp.astype(np.float64) + (0.0 if la is None else la)
        ln = a.max(axis=1) + np.log(np.exp(a - a.max(axis=1, keepdims=True)).sum(axis=1))
        got = sky.map_entropy(dev(lp), None if la is None else dev(la), dev(ln))
        assert got.dtype == F64 and tuple(got.shape) == (C,)
        for c in range(C):
            want = np_entropy(lp[c], None if la is None else (la[c] if la.ndim == 2 else la), ln[c])
            err = abs(host(got)[c] - want)
            print("M = %d %s row %d: entropy %.6f, |d| %.2e (bar %.2e)" % (M, dtype, c, want, err, M * 2.0 ** -52 * max(1.0, abs(want))))
            assert err <= M * 2.0 ** -52 * max(1.0, abs(want)) + 4 * 2.0 ** -52
        if la is not None and la.ndim == 2:                  # a row alone: the same bits
            assert torch.equal(sky.map_entropy(dev(lp[1:2]), dev(la[1:2]), dev(ln[1:2])), got[1:2])


# ---------------------------------------------------------------------------------------------- pdf.sky_map_adaptive
def np_log_area(ids):
    return np.array([LOG_BASE_AREA - float(order_of(u)) * LOG_4 for u in ids])


ADAPTIVE_KEYS = {"uniq", "log_prob", "log_area", "log_norm", "entropy", "map_uniq", "map_direction", "map_log_prob"}


@pytest.mark.parametrize("name,dtype", [("f_s2", F64), ("v_s2", F64), ("c3_e4s2e4", F64), ("c3_e4s2e4", F32), ("f_s2_cond_ff", F64),
                                        ("f_s2_cond_ff", F32)],
                         ids=["f_s2-f64", "v_s2-f64", "c3_e4s2e4-f64", "c3_e4s2e4-f32", "f_s2_cond_ff-f64", "f_s2_cond_ff-f32"])
def test_sky_map_adaptive(name, dtype):
    from jammy_flows_amd import sky
    base_order, rounds, M0, K = 1, 3, 48, 12
    M = M0 + 3 * K * rounds
    assert M == 156
    fx = fixture_io.load(name)
    pdf = build_product(fx, dtype)
    k = pdf.pdf_defs_list.index("s2")
    S = 8
    cond = to_dev(fx["cond"][:3], dtype) if "cond" in fx else None
    C = 1 if cond is None else 3
    z = to_dev(fx["z"][:S * C], dtype) if k > 0 else None
    labels = to_dev(fx["sample_x"][:C], dtype)[:, slice(*pdf.target_dim_indices[k])]
    if name == "v_s2":                                      # (C, 3) vectors instead of (C, 2) angles
        labels = torch.stack([torch.sin(labels[:, 0]) * torch.cos(labels[:, 1]), torch.sin(labels[:, 0]) * torch.sin(labels[:, 1]),
                              torch.cos(labels[:, 0])], dim=1)
    kw = dict(conditional_input=cond, samplesize=S, predefined_base=z)
    mkw = dict(conditional_input=cond, samplesize=S, force_embedding_coordinates=True, predefined_base=z)
    got = pdf.sky_map_adaptive(base_order, rounds, labels=labels, credible_masses=SKY_QS, **kw)

    # (a) keys, shapes, types
    assert set(got) == ADAPTIVE_KEYS | {"levels", "level_masses", "areas", "label_cell", "label_log_prob", "coverage"}
    assert all(v.is_cuda for v in got.values())
    for key, shape, want_dtype in (("uniq", (C, M), torch.int64), ("log_prob", (C, M), dtype), ("log_area", (C, M), F64), ("log_norm", (C,), F64),
                                   ("entropy", (C,), F64), ("map_uniq", (C,), torch.int64), ("map_direction", (C, 3), dtype),
                                   ("map_log_prob", (C,), dtype), ("levels", (C, 3), dtype), ("level_masses", (C, 3), F64), ("areas", (C, 3), F64),
                                   ("label_cell", (C,), torch.int64), ("label_log_prob", (C,), dtype), ("coverage", (C,), F64)):
        assert tuple(got[key].shape) == shape and got[key].dtype == want_dtype, key
    plain = pdf.sky_map_adaptive(base_order, rounds, **kw)
    assert set(plain) == ADAPTIVE_KEYS and torch.equal(plain["uniq"], got["uniq"]) and same_bits(plain["log_prob"], got["log_prob"])

    # (b) no rounds: sky_map's bits
    flat = pdf.sky_map(base_order, credible_masses=SKY_QS, **kw)
    none = pdf.sky_map_adaptive(base_order, 0, credible_masses=SKY_QS, **kw)
    assert same_bits(none["log_prob"], flat["log_prob"]) and torch.equal(none["levels"], flat["levels"])
    assert torch.equal(none["uniq"], sky.uniq_of(base_order, torch.arange(M0, device="cuda"))[None].expand(C, M0))

    # (c) a replay: numpy selection, Python ids, the same marginal_log_prob at the new centres
    ids = [list(range(4 * 4 ** base_order, 4 * 4 ** base_order + M0)) for _ in range(C)]
    lp = [list(r) for r in host(flat["log_prob"])]
    margins = []                                             # (g) per round and row: (smallest key split, largest key left)
    for _ in range(rounds):
        tile = np.array(lp, dtype=NP[dtype])
        log_area = np.stack([np_log_area(r) for r in ids])
        sel = np_select(tile, log_area, K)
        key = tile.astype(np.float64) + log_area
        new_ids, new_lp, new_cols = [], [], []
        for c in range(C):
            left = np.setdiff1d(np.arange(len(ids[c])), sel[c])
            margins.append((key[c, sel[c]].min(), key[c, left].max()))
            a, b, n = py_expand(ids[c], lp[c], sel[c].tolist())
            new_ids.append(a), new_lp.append(b), new_cols.append(n)
        children = np.array([[new_ids[c][i] for i in new_cols[c]] for c in range(C)], dtype=np.int64)
        vals = host(pdf.marginal_log_prob(k, sky.cell_centres(dev(children), dtype=dtype), **mkw))
        for c in range(C):
            for j, i in enumerate(new_cols[c]):
                new_lp[c][i] = vals[c, j]
        ids, lp = new_ids, new_lp
    assert host(got["uniq"]).tolist() == ids
    assert np.array_equal(host(got["log_prob"]).view(np.uint8), np.array(lp, dtype=NP[dtype]).view(np.uint8))
    # (g) every cell that was split carried at least the mass of every cell of its row that was left
    assert all(lo >= hi for lo, hi in margins), margins
    for c in range(C):
        check_partition(ids[c])
    assert torch.equal(got["log_area"], sky.cell_log_area(got["uniq"]))
    print("%s: finest order %d after %d rounds from order %d" % (name, max(order_of(u) for r in ids for u in r), rounds, base_order))

    # (d) the densities at the centres
    centres = sky.cell_centres(got["uniq"], dtype=dtype)     # (C, M, 3)
    tile = got["log_prob"]
    if dtype == F64:
        oracle = build_oracle(fx)
        for c in range(C):
            if k == 0:
                rep = None if cond is None else np.repeat(fx["cond"][c:c + 1], M, axis=0)
                ref = oracle.forward(host(centres[c]), rep, force_embedding_coordinates=True)[0]
            else:
                _, samples = pdf.marginal_log_prob(k, centres[c], return_samples=True, **mkw)
                rows = host(samples)[:, None, :].repeat(M, axis=1)
                ea, eb = pdf.target_dim_indices_embedded[k]
                rows[:, :, ea:eb] = host(centres[c])[None]
                per = oracle_block_logp(oracle, rows.reshape(S * M, -1), k).reshape(S, M)
                ref = np.logaddexp.reduce(per, axis=0) - math.log(S)
            err = np.abs(host(tile)[c] - ref) / (1 + np.abs(ref))
            print("%s row %d: max |d log_prob| / (1 + |ref|) = %.3e" % (name, c, err.max()))
            assert err.max() <= 1e-7
    else:
        pdf64 = build_product(fx, F64)
        for c in range(C):
            c64 = centres[c].double()
            if k == 0:
                rep = None if cond is None else cond[c:c + 1].repeat(M, 1)
                ref = pdf64(c64, conditional_input=None if rep is None else rep.double(), force_embedding_coordinates=True)[0]
                e_pdf = float((pdf(centres[c], conditional_input=rep, force_embedding_coordinates=True)[0].double() - ref).abs().max())
            else:
                ref, samples = pdf64.marginal_log_prob(k, c64, samplesize=S, force_embedding_coordinates=True, predefined_base=z.double(),
                                                       return_samples=True)
                ref = ref[0]
                rows = samples[:, None, :].repeat(1, M, 1)
                ea, eb = pdf.target_dim_indices_embedded[k]
                rows[:, :, ea:eb] = c64[None]
                rows = rows.reshape(S * M, -1)
                e_pdf = float((pdf(rows.float(), force_embedding_coordinates=True)[0].double()
                               - pdf64(rows, force_embedding_coordinates=True)[0]).abs().max())
            e_map = float((tile[c].double() - ref).abs().max())
            print("%s float32 row %d: pdf() vs float64 %.3e, sky_map_adaptive vs float64 %.3e" % (name, c, e_pdf, e_map))
            assert e_map <= 2 * e_pdf

    # (e) the reductions against numpy on the device's own tile
    label_pix = host(sky.vec2pix(29, labels))
    lp_h, la_h, uniq_h = host(tile), host(got["log_area"]), host(got["uniq"])
    for c in range(C):
        what = "%s row %d" % (name, c)
        cell = int(got["label_cell"][c])
        assert 0 <= cell < M and start_of(ids[c][cell]) <= int(label_pix[c]) < start_of(ids[c][cell]) + 4 ** (29 - order_of(ids[c][cell]))
        want = recompute(lp_h[c], la_h[c], SKY_QS, cell)
        row = {key: host(got[key])[c] for key in ("log_norm", "levels", "level_masses", "areas", "coverage")}
        check_row(row, want, M, what)
        assert int(got["map_uniq"][c]) == uniq_h[c, want["argmax"]] and host(got["map_log_prob"])[c] == want["max"]
        assert torch.equal(got["map_direction"][c], sky.cell_centres(got["map_uniq"][c:c + 1], dtype=dtype)[0])
        assert host(got["label_log_prob"])[c] == lp_h[c, cell]
        ent = np_entropy(lp_h[c], la_h[c], want["log_norm"])
        assert abs(host(got["entropy"])[c] - ent) <= M * 2.0 ** -52 * max(1.0, abs(ent)) + 4 * 2.0 ** -52, what
        print("%s: log_norm %.5f, entropy %.5f, areas %s sr, coverage %.4f" % (what, row["log_norm"], ent, row["areas"], row["coverage"]))

    # (f) a conditional input alone: its row of the batch, bit for bit
    for c in range(C if C > 1 else 0):
        alone = pdf.sky_map_adaptive(base_order, rounds, conditional_input=cond[c:c + 1], samplesize=S, labels=labels[c:c + 1],
                                     credible_masses=SKY_QS)
        assert set(alone) == set(got)
        for key in got:
            assert same_bits(alone[key], got[key][c:c + 1]) if got[key].is_floating_point() else torch.equal(alone[key], got[key][c:c + 1]), (c, key)




def test_sky_map_adaptive_draws_its_base_samples_once():
    """behind another block and without predefined_base the base samples are drawn here, once, for the base map and every round: with the
    generator seeded the map is the one of the same draw passed in, bit for bit"""
    fx = fixture_io.load("c3_e4s2e4")
    pdf = build_product(fx, F64)
    k, S = pdf.pdf_defs_list.index("s2"), 8
    assert k > 0
    torch.manual_seed(11)
    got = pdf.sky_map_adaptive(1, 3, samplesize=S, credible_masses=SKY_QS)
    torch.manual_seed(11)
    z = torch.randn((S, pdf.total_base_dim), dtype=F64, device="cuda")
    want = pdf.sky_map_adaptive(1, 3, samplesize=S, credible_masses=SKY_QS, predefined_base=z)
    assert set(got) == set(want) == ADAPTIVE_KEYS | {"levels", "level_masses", "areas"}
    assert tuple(got["uniq"].shape) == (1, 156) and bool(torch.isfinite(got["log_norm"]).all())
    for key in got:
        assert same_bits(got[key], want[key]) if got[key].is_floating_point() else torch.equal(got[key], want[key]), key
    other = pdf.sky_map_adaptive(1, 3, samplesize=S)         # the next draw: another estimate of the same map
    assert not torch.equal(other["log_prob"], got["log_prob"])
