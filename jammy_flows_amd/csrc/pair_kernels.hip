// Pairwise marginal kernels: the S x S evaluation behind the marginal entropy of one sub-manifold (pdf.entropy_iterative, pdf.marginal_moments;
// reference main/default.py:2263-2454 and its chunked twin entropy_iterative).
//
// For G groups (conditional inputs) of S samples each, targets x[G*S, w] (default coordinates of block k) and parameter rows params[G*S, P]
// (the amortisation MLP's output for (cond_g, embed(x_<k of sample j)); row stride 0 = one permanent row):
//
//     tile[g, j, i - i0] = logN(f^-1(x[g,i]; params[g,j])) + log_det(x[g,i]; params[g,j])          (pair kernels, one launch)
//     out[g, i]          = add[g, i] + logsumexp_j tile[g, j, i - i0] - log S                      (pair_reduce_kernel)
//
// Work distribution: workgroup blockIdx.x owns ONE parameter row (g, j).  It stages and derives that row in LDS exactly as the broadcast
// launches of gf_kernels.hip / manifold_kernels.hip do for their one row per launch -- here the row is chosen per workgroup -- and then walks
// the targets i0 .. i1 of group g against it (row tiles blockIdx.y, blockIdx.y + gridDim.y, ...).  The parameters are read from HBM once per
// (g, j), the S x S values never exist wider than one scalar per pair, and a pair's value depends on nothing but its own target and parameter
// row.  The reduction walks j = 0 .. S-1 sequentially for each (g, i): its order is fixed, so out[g, i] carries the same bits for every
// i-range, every number of groups in the launch and every grid (the project's row-independence rule).  No floating-point atomics.
//
// The same kernels evaluate RECTANGULAR tiles (jf_grid_gf / jf_grid_mchain / jf_grid_reduce, behind pdf.log_prob_on_grid and
// pdf.marginal_log_prob): J parameter rows against N targets per group, the targets per group or shared by all groups, the tile returned
// instead of reduced (PairDims below).  The pairwise entry points are the case J = N = S.
#include <type_traits>

#include "jf_gfb.h"
#include "jf_mchain_plan.h"

namespace jf {

int gf_pair_fill_f32(GfChainArgs<float>& a, const float* p, int32_t D, int32_t n, const jf_gf_layer* L, size_t& lds);     // gf_kernels.hip
int gf_pair_fill_f64(GfChainArgs<double>& a, const double* p, int32_t D, int32_t n, const jf_gf_layer* L, size_t& lds);
static int gf_pair_fill(GfChainArgs<float>& a, const float* p, int32_t D, int32_t n, const jf_gf_layer* L, size_t& lds) { return gf_pair_fill_f32(a, p, D, n, L, lds); }
static int gf_pair_fill(GfChainArgs<double>& a, const double* p, int32_t D, int32_t n, const jf_gf_layer* L, size_t& lds) { return gf_pair_fill_f64(a, p, D, n, L, lds); }

// J parameter rows against N targets per group.  The pairwise entry points are the square case J = N = S with per-group targets (xgs = S);
// the grid entry points take any J and N and, with xgs = 0, one target set shared by all groups.
struct PairDims {
    int J;                   // parameter rows per group
    int N;                   // targets per group
    int64_t xgs;             // rows between the target sets of consecutive groups (N: per-group targets, 0: one set shared by all groups)
    int i0, ni;              // targets i0 .. i0 + ni of every group
};

// workgroups a launch aims for before it splits the target walk over blockIdx.y (a few rounds of the chip's resident workgroups)
constexpr int PAIR_TARGET_BLOCKS = 8192;
static unsigned pair_grid_y(int64_t rows_xj, int64_t n_tiles) {
    int64_t y = (PAIR_TARGET_BLOCKS + rows_xj - 1) / rows_xj;
    if (y > n_tiles) y = n_tiles;
    if (y > 65535) y = 65535;
    return (unsigned)(y < 1 ? 1 : y);
}

// ---------------------------------------------------------------------------------------------------------- 'g' chains
// lane = (target, coordinate) as gf_chain_kernel's broadcast regime: G = next power of two >= D lanes own one target, 256 / G targets per tile
template <typename T, int G>
__global__ void __launch_bounds__(256, sizeof(T) == 8 ? 2 : 4) pair_gf_kernel(const GfChainArgs<T> a, const PairDims pd, T* __restrict__ tile_out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* lds = reinterpret_cast<T*>(smem_raw);
    constexpr int R = 256 / G;
    const int tid = threadIdx.x;
    const int g = tid & (G - 1), r = tid >> Log2<G>::v;
    const int D = a.D;
    const bool live = g < D, leader = g == 0;
    const int d = live ? g : D - 1;
    T* spl_tab = lds + a.tab_offset;
    const int64_t gj = blockIdx.x;                        // = group * J + j
    derive_broadcast_from<T>(lds, a, a.params + gj * a.ps);
    const int64_t grp = gj / pd.J;
    const T* xg = a.x + (grp * pd.xgs + pd.i0) * a.xs;
    T* out = tile_out + gj * pd.ni;
    const int n_layers = __builtin_amdgcn_readfirstlane(a.n_layers);

    for (int row0 = (int)blockIdx.y * R; row0 < pd.ni; row0 += (int)gridDim.y * R) {
        const int row = row0 + r;
        const bool row_valid = row < pd.ni;
        const int rrow = row_valid ? row : pd.ni - 1;
        T x = xg[(int64_t)rrow * a.xs + d];
        T ld = T(0);
        for (int l = n_layers - 1; l >= 0; --l) {
            const GfLayerDev<T> o = a.L[l];
            const T* p = lds + l * a.tile_stride + d;
            if (o.model_offset) x -= p[0];                                                   // euclidean_base.py:40-45
            x = gfg_rotate_inv<T, G, false>(p, o, D, live, x);
            if (o.stretch == JF_GF_STRETCH_RQ_SPLINES) {
                const T* pr = p - d;
                T* tab = spl_tab + tid * a.spline_tab;
                const SplineOut<T> sr = spline_linext<T>(pr + o.off_mean + d * o.K, pr + o.off_lw + d * o.K, pr + o.off_ln + d * (o.K + 1),
                                                         pr + o.off_box + d * 4, o.K, tab, x, false);
                x = sr.y;
                ld += group_sum<T, G>(live ? sr.lad : T(0));
            } else {
                const MixQ<T> q = gfg_mixture<T, false>(p, o, D, x);
                const IcdfOut<T> s = gf_icdf<T>(o.inv_type, q);
                x = s.y;
                ld += group_sum<T, G>(live ? s.logd : T(0));
            }
        }
        const T sb = group_sum<T, G>(live ? gfb_base_term<T>(x) : T(0));
        const T v = sb + ld;
        if (row_valid && leader) out[row] = v;
        const T bad = group_max<T, G>((live && !M<T>::finite(x)) ? T(1) : T(0));
        status_add(a.status, JF_STATUS_NONFINITE, row_valid && leader && (bad > T(0) || !M<T>::finite(ld)));
    }
}

template <typename T, int G> static int launch_pair_gf(const GfChainArgs<T>& a, const PairDims& pd, int64_t n_rows, size_t lds, T* tile, hipStream_t st) {
    auto k = pair_gf_kernel<T, G>;
    allow_lds(k, lds);
    constexpr int R = 256 / G;
    const int64_t n_tiles = (pd.ni + R - 1) / R;
    jf::launch(k, dim3((unsigned)n_rows, pair_grid_y(n_rows, n_tiles)), dim3(256), lds, st, a, pd, tile);
    return check_launch();
}

// Classic stretch, D <= 8: lane = TARGET, the row walk of gfb_chain_inv_body (jf_gfb.h) on the workgroup's own parameter row -- the derived
// (mean, 1 / width, pi, pi / width) records of a component are one wave-uniform LDS read per 64 targets, the Householder dot products and the
// sums over the coordinates are register arithmetic.  Same device functions per coordinate (gfb_mix_sums, gfb_scaled_rows, gf_icdf), so a pair
// value carries the bits the lane = row broadcast launch of gf_kernels.hip gives the same target and parameter row.  Which of the two pair
// kernels runs follows the chain (D, stretch) alone, never the sizes of the call.
template <typename T, int D>
__global__ void __launch_bounds__(256) pair_gfb_kernel(const GfChainArgs<T> a, const PairDims pd, T* __restrict__ tile_out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* lds = reinterpret_cast<T*>(smem_raw);
    const int tid = threadIdx.x;
    const int64_t gj = blockIdx.x;
    derive_broadcast_from<T>(lds, a, a.params + gj * a.ps);
    const int n_layers = __builtin_amdgcn_readfirstlane(a.n_layers);
    int max_k = 1;
    for (int l = 0; l < n_layers; ++l) max_k = a.L[l].K > max_k ? a.L[l].K : max_k;
    const int pstride = __builtin_amdgcn_readfirstlane(max_k) * D;
    GfPack<T>* pack = reinterpret_cast<GfPack<T>*>(lds + a.tab_offset);
    for (int l = 0; l < n_layers; ++l) {
        const GfLayerDev<T> o = a.L[l];
        const T* row = lds + l * a.tile_stride;
        for (int j = tid; j < o.K * D; j += 256) {
            const int d = j / o.K, k = j - d * o.K;
            GfPack<T> e;
            e.mean = row[o.off_mean + k * D + d];
            e.iw = row[o.off_lw + k * D + d];
            e.pi = o.fit_norm ? row[o.off_ln + k * D + d] : M<T>::rcp(T(o.K));
            e.piw = e.pi * e.iw;
            if constexpr (sizeof(T) == 4) e.iw *= T(-1.4426950408889634);     // (the float32 records carry -log2(e) / width: jf_gfb.h)
            pack[l * pstride + j] = e;
        }
    }
    __syncthreads();
    const int64_t grp = gj / pd.J;
    const T* xg = a.x + (grp * pd.xgs + pd.i0) * a.xs;
    T* out = tile_out + gj * pd.ni;
    int n_bad = 0;
    const int step = (int)gridDim.y * 256;
    for (int row0 = (int)blockIdx.y * 256; row0 < pd.ni; row0 += step) {
        const int row = row0 + tid;
        const bool row_valid = row < pd.ni;
        const int rrow = row_valid ? row : pd.ni - 1;
        T x[D];
#pragma unroll
        for (int d = 0; d < D; ++d) x[d] = xg[(int64_t)rrow * a.xs + d];
        T ld = T(0);
        for (int l = n_layers - 1; l >= 0; --l) {
            const GfLayerDev<T> o = a.L[l];
            const T* prow = lds + l * a.tile_stride;
            if (o.model_offset) {
#pragma unroll
                for (int d = 0; d < D; ++d) x[d] -= prow[d];
            }
            for (int i = 0; i < o.hh; ++i) {
                const T* v = prow + o.off_rot + i * D;
                const T dot = gfb_hh_dot<T, D>(v, x);
#pragma unroll
                for (int d = 0; d < D; ++d) x[d] = gfb_hh_apply<T>(x[d], v[d], dot);
            }
            const GfPack<T>* pk = pack + l * pstride;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const GfPack<T>* pdd = pk + d * o.K;
                T C, S, P;
                gfb_mix_sums<T>(pdd, o.K, x[d], C, S, P);
                MixQ<T> q;
                q.lc = M<T>::log_fast(C); q.ls = M<T>::log_fast(S); q.lp = M<T>::log_fast(P);
                q.cdf = C; q.sf = S;
                const bool under = !(C > M<T>::TINY && S > M<T>::TINY && P > M<T>::TINY);
                if (__any(under)) {                        // wave-uniform branch
                    if (o.K <= 16) {
                        gfb_scaled_rows<T>(pdd, o.K, x[d], under, q);
                    } else {
                        const MixQ<T> qs = gfg_mixture_scaled<T, false>(prow + d, o, D, x[d], T(0));
                        if (under) q = qs;
                    }
                }
                const IcdfOut<T> sy = gf_icdf<T>(o.inv_type, q);
                x[d] = sy.y;
                ld += sy.logd;
            }
        }
        T sb = T(0);
        bool bad = !M<T>::finite(ld);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            sb += gfb_base_term<T>(x[d]);
            bad = bad || !M<T>::finite(x[d]);
        }
        if (row_valid) out[row] = sb + ld;
        n_bad += (row_valid && bad) ? 1 : 0;
    }
    if (a.status != nullptr) {                            // pairs with a non-finite value: one atomic per wave, after the walk
        for (int off = 32; off > 0; off >>= 1) n_bad += __shfl_xor(n_bad, off, 64);
        if ((tid & 63) == 0 && n_bad) atomicAdd(a.status + JF_STATUS_NONFINITE, n_bad);
    }
}

template <typename T, int D> static int launch_pair_gfb(const GfChainArgs<T>& a, const PairDims& pd, int64_t n_rows, size_t lds, T* tile, hipStream_t st) {
    auto k = pair_gfb_kernel<T, D>;
    allow_lds(k, lds);
    const int64_t n_tiles = (pd.ni + 255) / 256;
    jf::launch(k, dim3((unsigned)n_rows, pair_grid_y(n_rows, n_tiles)), dim3(256), lds, st, a, pd, tile);
    return check_launch();
}

// ---------------------------------------------------------------------------------------------------------- reduction over j
// out[g * ostride + o0 + i] = add[same] + log sum_j exp(tile[g, j, i] + logw[g * J + j]); WEIGHTED = false: uniform weights 1 / J, computed as
// m + log(s) - log(J).  j runs 0 .. J-1 in this order for every (g, i).  torch.logsumexp's special values over the terms tile + logw: an
// infinite maximum is replaced by 0 in the subtraction, so any NaN term gives NaN, else any +inf gives +inf, else all -inf gives -inf; a finite
// maximum leaves every operation as it was.
template <typename T, bool WEIGHTED>
__global__ void __launch_bounds__(256) pair_reduce_kernel(const T* __restrict__ tile, const T* __restrict__ logw, const T* __restrict__ add,
                                                          int64_t n_groups, int J, int ni, int64_t ostride, int o0, T* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_groups * ni) return;
    const int64_t grp = t / ni;
    const int il = (int)(t - grp * ni);
    const T* p = tile + grp * J * ni + il;                // element j at p[j * ni]: consecutive lanes read consecutive words
    const T* w = WEIGHTED ? logw + grp * J : nullptr;
    T m = -INFINITY;
    for (int j = 0; j < J; ++j) m = M<T>::max(m, WEIGHTED ? p[(int64_t)j * ni] + w[j] : p[(int64_t)j * ni]);
    if (!M<T>::finite(m)) m = T(0);                       // (m is never NaN: fmax skips NaN)
    T s = T(0);
    for (int j = 0; j < J; ++j) s += M<T>::exp((WEIGHTED ? p[(int64_t)j * ni] + w[j] : p[(int64_t)j * ni]) - m);
    const int64_t o = grp * ostride + o0 + il;
    const T v = WEIGHTED ? m + M<T>::log(s) : m + M<T>::log(s) - M<T>::log(T(J));
    out[o] = add ? add[o] + v : v;
}
template <typename T>
static int pair_reduce(const T* tile, const T* logw, const T* add, int64_t n_groups, int J, int ni, int64_t ostride, int o0, T* out, hipStream_t st) {
    const int64_t n = n_groups * ni;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (logw) jf::launch(pair_reduce_kernel<T, true>, grid, dim3(256), 0, st, tile, logw, add, n_groups, J, ni, ostride, o0, out);
    else jf::launch(pair_reduce_kernel<T, false>, grid, dim3(256), 0, st, tile, logw, add, n_groups, J, ni, ostride, o0, out);
    return check_launch();
}

static int pair_dims(int64_t n_groups, int32_t J, int32_t N, int64_t xgs, int32_t i0, int32_t i1, PairDims& pd) {
    if (n_groups < 0 || J < 1 || i0 < 0 || i1 < i0 || i1 > N || !(xgs == 0 || xgs >= i1)) return JF_ERR_BADARG;
    if (n_groups > (int64_t)0x7fffffff || n_groups * (int64_t)J > (int64_t)0x7fffffff) return JF_ERR_UNSUPPORTED;   // (one workgroup per parameter row: grid.x)
    pd.J = J; pd.N = N; pd.xgs = xgs; pd.i0 = i0; pd.ni = i1 - i0;
    return JF_OK;
}

// the tile alone: tile[(g * J + j) * ni + (i - i0)] for the targets [i0, i1) of every group
template <typename T>
static int grid_gf(const T* x, int64_t xs, int64_t xgs, const T* params, int64_t ps, int64_t n_groups, int32_t J, int32_t N, int32_t i0, int32_t i1,
                   int32_t D, int32_t n_layers, const jf_gf_layer* layers, T* tile, int32_t* status, void* stream) {
    if (!x || !params || !tile || xs < D || ps < 0) return JF_ERR_BADARG;
    PairDims pd{};
    int rc = pair_dims(n_groups, J, N, xgs, i0, i1, pd);
    if (rc != JF_OK) return rc;
    GfChainArgs<T> a{};
    size_t lds = 0;
    rc = gf_pair_fill(a, params, D, n_layers, layers, lds);
    if (rc != JF_OK) return rc;
    if (n_groups == 0 || pd.ni == 0) return JF_OK;
    a.x = x; a.xs = xs; a.ps = ps; a.B = pd.ni; a.status = status;
    const int64_t n_rows = n_groups * J;
    hipStream_t st = (hipStream_t)stream;
    // classic stretch, D <= 8, the component records fit: the lane = target walk (as gf_kernels.hip picks its lane = row broadcast kernel)
    bool classic = true;
    int max_k = 1;
    for (int l = 0; l < n_layers; ++l) {
        classic = classic && a.L[l].stretch == JF_GF_STRETCH_CLASSIC;
        max_k = a.L[l].K > max_k ? a.L[l].K : max_k;
    }
    const size_t lds_rows = ((size_t)a.tab_offset + (size_t)n_layers * max_k * D * 4) * sizeof(T);
    if (classic && D <= 8 && lds_rows <= JF_LDS_WG_MAX) {
        switch (D) {
            case 1: rc = launch_pair_gfb<T, 1>(a, pd, n_rows, lds_rows, tile, st); break;
            case 2: rc = launch_pair_gfb<T, 2>(a, pd, n_rows, lds_rows, tile, st); break;
            case 3: rc = launch_pair_gfb<T, 3>(a, pd, n_rows, lds_rows, tile, st); break;
            case 4: rc = launch_pair_gfb<T, 4>(a, pd, n_rows, lds_rows, tile, st); break;
            case 5: rc = launch_pair_gfb<T, 5>(a, pd, n_rows, lds_rows, tile, st); break;
            case 6: rc = launch_pair_gfb<T, 6>(a, pd, n_rows, lds_rows, tile, st); break;
            case 7: rc = launch_pair_gfb<T, 7>(a, pd, n_rows, lds_rows, tile, st); break;
            default: rc = launch_pair_gfb<T, 8>(a, pd, n_rows, lds_rows, tile, st); break;
        }
        return rc;
    }
    const int G = D <= 1 ? 1 : D <= 2 ? 2 : D <= 4 ? 4 : D <= 8 ? 8 : D <= 16 ? 16 : D <= 32 ? 32 : 64;
    switch (G) {
        case 1: rc = launch_pair_gf<T, 1>(a, pd, n_rows, lds, tile, st); break;
        case 2: rc = launch_pair_gf<T, 2>(a, pd, n_rows, lds, tile, st); break;
        case 4: rc = launch_pair_gf<T, 4>(a, pd, n_rows, lds, tile, st); break;
        case 8: rc = launch_pair_gf<T, 8>(a, pd, n_rows, lds, tile, st); break;
        case 16: rc = launch_pair_gf<T, 16>(a, pd, n_rows, lds, tile, st); break;
        case 32: rc = launch_pair_gf<T, 32>(a, pd, n_rows, lds, tile, st); break;
        default: rc = launch_pair_gf<T, 64>(a, pd, n_rows, lds, tile, st); break;
    }
    return rc;
}

// the pairwise entry point: the square case J = N = S of grid_gf with per-group targets, reduced over j with uniform weights
template <typename T>
static int pair_gf(const T* x, int64_t xs, const T* params, int64_t ps, int64_t n_groups, int32_t S, int32_t i0, int32_t i1, int32_t D, int32_t n_layers,
                   const jf_gf_layer* layers, const T* add, T* tile, T* out, int32_t* status, void* stream) {
    if (!x || !params || !tile || !out || xs < D || ps < 0) return JF_ERR_BADARG;
    const int rc = grid_gf<T>(x, xs, S, params, ps, n_groups, S, S, i0, i1, D, n_layers, layers, tile, status, stream);
    if (rc != JF_OK || n_groups == 0 || i1 == i0) return rc;
    return pair_reduce<T>(tile, nullptr, add, n_groups, S, i1 - i0, S, i0, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------- manifold chains
// one wave per workgroup, lane = target (as mchain_kernel).  Every layer's raw row of the workgroup's (g, j) is staged once, and where the
// family's knot table does not depend on the target (Fam::build) it is built once per layer and workgroup, as mchain_kernel does for its
// broadcast case; the other spline families keep lane-private tables.
template <typename T, typename CLayer> struct MPairArgs {
    const T* x; int64_t xs;
    const T* params; int64_t ps;
    int n_layers;
    int dim;
    int tile_stride;
    int scratch;             // per-lane elements of the emitted-parameter scratch ('f' correlated)
    int tab;                 // elements of one knot table (0: no spline in the chain)
    int shared_tab;          // one table per (workgroup, layer) instead of one per lane
    int col0[JF_MAX_MCHAIN];
    int ncols[JF_MAX_MCHAIN];
    CLayer L[JF_MAX_MCHAIN];
    int32_t* status;
};

template <typename T, class Fam>
__global__ void __launch_bounds__(64) pair_mchain_kernel(const MPairArgs<T, typename Fam::CLayer> a, const PairDims pd, T* __restrict__ tile_out) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T* rows = reinterpret_cast<T*>(smem_raw);
    const int tid = threadIdx.x;
    constexpr bool CAN_SHARE = fam_has_build<Fam>::value;
    const bool shared = CAN_SHARE && a.shared_tab != 0;  // uniform
    T* tabs = rows + a.n_layers * a.tile_stride;
    T* corr = tabs + (shared ? a.n_layers : 64) * a.tab + tid * a.scratch;
    const int64_t gj = blockIdx.x;
    const T* prow_g = a.params + gj * a.ps;
    for (int l = 0; l < a.n_layers; ++l)
        for (int j = tid; j < a.ncols[l]; j += 64) rows[l * a.tile_stride + j] = prow_g[a.col0[l] + j];
    __syncthreads();
    if constexpr (CAN_SHARE) {
        if (shared) {
            for (int l = 0; l < a.n_layers; ++l)          // (uniform loop: the layer descriptors stay scalar loads)
                if (tid == 0) Fam::template build<T>(a.L[l], rows + l * a.tile_stride, tabs + l * a.tab);
            __syncthreads();
        }
    }
    const int64_t grp = gj / pd.J;
    const T* xg = a.x + (grp * pd.xgs + pd.i0) * a.xs;
    T* out = tile_out + gj * pd.ni;

    int n_bad = 0, n_oob = 0, n_nonconv = 0;
    LaneCtx<T> ctx;
    ctx.corr = corr;
    ctx.bins = nullptr;
    const int step = (int)gridDim.y * 64;
    for (int row0 = (int)blockIdx.y * 64; row0 < pd.ni; row0 += step) {
        const int row = row0 + tid;
        const bool active = row < pd.ni;
        const int rrow = active ? row : pd.ni - 1;
        T x[3] = {T(0), T(0), T(0)};
#pragma unroll
        for (int d = 0; d < Fam::DIM; ++d) x[d] = xg[(int64_t)rrow * a.xs + d];
        T ld = T(0);
        ctx.bin_i = 0;
        ctx.oob = ctx.nonconv = ctx.nonfinite = false;
        ctx.lane_valid = active;
        for (int l = a.n_layers - 1; l >= 0; --l) {
            ctx.tab = shared ? tabs + l * a.tab : tabs + tid * a.tab;
            ctx.tab_built = shared;
            Fam::template apply<T, false>(a.L[l], rows + l * a.tile_stride, x, ld, ctx);
        }
        bool bad = !M<T>::finite(ld);
        T s = T(0);
#pragma unroll
        for (int d = 0; d < Fam::DIM; ++d) {
            bad = bad || !M<T>::finite(x[d]);
            s += T(-0.5) * x[d] * x[d] - M<T>::HALF_LN_2PI;
        }
        if (active) out[row] = s + ld;
        n_bad += (active && (bad || ctx.nonfinite)) ? 1 : 0;
        n_oob += (active && ctx.oob) ? 1 : 0;
        n_nonconv += (active && ctx.nonconv) ? 1 : 0;
    }
    // the status words count (target, parameter row) pairs; one wave-aggregated atomic per word and workgroup, after the walk
    if (a.status != nullptr) {
        for (int off = 32; off > 0; off >>= 1) {
            n_bad += __shfl_xor(n_bad, off, 64); n_oob += __shfl_xor(n_oob, off, 64); n_nonconv += __shfl_xor(n_nonconv, off, 64);
        }
        if (tid == 0) {
            if (n_bad) atomicAdd(a.status + JF_STATUS_NONFINITE, n_bad);
            if (n_oob) atomicAdd(a.status + JF_STATUS_OUT_OF_RANGE, n_oob);
            if (n_nonconv) atomicAdd(a.status + JF_STATUS_NONCONVERGED, n_nonconv);
        }
    }
}

template <typename T, class Fam>
static int grid_mchain(const T* x, int64_t xs, int64_t xgs, const T* params, int64_t ps, int64_t n_groups, int32_t J, int32_t N, int32_t i0, int32_t i1,
                       int32_t n_layers, const typename Fam::CLayer* layers, T* tile, int32_t* status, void* stream) {
    if (!x || !tile || xs < Fam::DIM || ps < 0) return JF_ERR_BADARG;
    PairDims pd{};
    int rc = pair_dims(n_groups, J, N, xgs, i0, i1, pd);
    if (rc != JF_OK) return rc;
    ChainPlan<Fam> plan;
    rc = plan_chain<Fam>(layers, n_layers, plan);
    if (rc != JF_OK) return rc;
    if (plan.P > 0 && !params) return JF_ERR_BADARG;
    MPairArgs<T, typename Fam::CLayer> a{};
    a.x = x; a.xs = xs; a.params = params; a.ps = ps; a.n_layers = n_layers; a.dim = plan.dim; a.status = status;
    for (int l = 0; l < n_layers; ++l) { a.L[l] = layers[l]; a.col0[l] = plan.col0[l]; a.ncols[l] = plan.ncols[l]; }
    a.tile_stride = padded_stride<T>(plan.max_row > 0 ? plan.max_row : 1);
    a.scratch = plan.corr;
    a.tab = plan.tab;
    a.shared_tab = (fam_has_build<Fam>::value && a.tab > 0) ? 1 : 0;
    const size_t lds = ((size_t)n_layers * a.tile_stride + (size_t)(a.shared_tab ? n_layers : 64) * a.tab + (size_t)64 * a.scratch) * sizeof(T);
    if (lds > JF_LDS_WG_MAX) return JF_ERR_UNSUPPORTED;
    if (n_groups == 0 || pd.ni == 0) return JF_OK;
    auto k = pair_mchain_kernel<T, Fam>;
    allow_lds(k, lds);
    const int64_t n_rows = n_groups * J, n_tiles = (pd.ni + 63) / 64;
    hipStream_t st = (hipStream_t)stream;
    jf::launch(k, dim3((unsigned)n_rows, pair_grid_y(n_rows, n_tiles)), dim3(64), lds, st, a, pd, tile);
    return check_launch();
}

template <typename T>
static int grid_mchain_any(int32_t fam, const T* x, int64_t xs, int64_t xgs, const T* p, int64_t ps, int64_t n_groups, int32_t J, int32_t N, int32_t i0,
                           int32_t i1, int32_t n, const void* L, T* tile, int32_t* status, void* stream) {
    switch (fam) {
        case 'r': return grid_mchain<T, RFam>(x, xs, xgs, p, ps, n_groups, J, N, i0, i1, n, static_cast<const jf_r_layer*>(L), tile, status, stream);
        case 'o': return grid_mchain<T, OFam>(x, xs, xgs, p, ps, n_groups, J, N, i0, i1, n, static_cast<const jf_o_layer*>(L), tile, status, stream);
        case 'm': return grid_mchain<T, MFam>(x, xs, xgs, p, ps, n_groups, J, N, i0, i1, n, static_cast<const jf_m_layer*>(L), tile, status, stream);
        case 'f': return grid_mchain<T, FFam>(x, xs, xgs, p, ps, n_groups, J, N, i0, i1, n, static_cast<const jf_f_layer*>(L), tile, status, stream);
        case 'v':
            // the reference asserts float64 for 'v' (exponential_map_s2.py:450, 493): no float32 kernel, as for jf_v_chain_*
            if constexpr (sizeof(T) == 8) return grid_mchain<T, VFam>(x, xs, xgs, p, ps, n_groups, J, N, i0, i1, n, static_cast<const jf_v_layer*>(L), tile, status, stream);
            else return JF_ERR_UNSUPPORTED;
        default: return JF_ERR_UNSUPPORTED;
    }
}

// the pairwise entry point: the square case J = N = S of grid_mchain with per-group targets, reduced over j with uniform weights
template <typename T>
static int pair_mchain_any(int32_t fam, const T* x, int64_t xs, const T* p, int64_t ps, int64_t n_groups, int32_t S, int32_t i0, int32_t i1, int32_t n,
                           const void* L, const T* add, T* tile, T* out, int32_t* status, void* stream) {
    const bool known = fam == 'r' || fam == 'o' || fam == 'm' || fam == 'f' || (fam == 'v' && sizeof(T) == 8);
    if (known && !out) return JF_ERR_BADARG;
    const int rc = grid_mchain_any<T>(fam, x, xs, S, p, ps, n_groups, S, S, i0, i1, n, L, tile, status, stream);
    if (rc != JF_OK || n_groups == 0 || i1 == i0) return rc;
    return pair_reduce<T>(tile, nullptr, add, n_groups, S, i1 - i0, S, i0, out, (hipStream_t)stream);
}

template <typename T>
static int grid_reduce(const T* tile, const T* logw, const T* add, int64_t n_groups, int32_t J, int32_t ni, T* out, void* stream) {
    if (!tile || !out || n_groups < 0 || J < 1 || ni < 0) return JF_ERR_BADARG;
    if (n_groups > (int64_t)0x7fffffff || n_groups * (int64_t)J > (int64_t)0x7fffffff || n_groups * (int64_t)ni > (int64_t)0x7fffffff * 256)
        return JF_ERR_UNSUPPORTED;                        // (the limit of jf_grid_gf / jf_grid_mchain on the tile; one thread per (g, i): grid.x)
    if (n_groups == 0 || ni == 0) return JF_OK;
    return pair_reduce<T>(tile, logw, add, n_groups, J, ni, ni, 0, out, (hipStream_t)stream);
}

}  // namespace jf

extern "C" {
int jf_pair_gf_f32(const float* x, int64_t xs, const float* p, int64_t ps, int64_t n_groups, int32_t S, int32_t i0, int32_t i1, int32_t D, int32_t n,
                   const jf_gf_layer* L, const float* add, float* tile, float* out, int32_t* st, void* s) {
    return jf::pair_gf<float>(x, xs, p, ps, n_groups, S, i0, i1, D, n, L, add, tile, out, st, s);
}
int jf_pair_gf_f64(const double* x, int64_t xs, const double* p, int64_t ps, int64_t n_groups, int32_t S, int32_t i0, int32_t i1, int32_t D, int32_t n,
                   const jf_gf_layer* L, const double* add, double* tile, double* out, int32_t* st, void* s) {
    return jf::pair_gf<double>(x, xs, p, ps, n_groups, S, i0, i1, D, n, L, add, tile, out, st, s);
}
int jf_pair_mchain_f32(int32_t fam, const float* x, int64_t xs, const float* p, int64_t ps, int64_t n_groups, int32_t S, int32_t i0, int32_t i1,
                       int32_t n, const void* L, const float* add, float* tile, float* out, int32_t* st, void* s) {
    return jf::pair_mchain_any<float>(fam, x, xs, p, ps, n_groups, S, i0, i1, n, L, add, tile, out, st, s);
}
int jf_pair_mchain_f64(int32_t fam, const double* x, int64_t xs, const double* p, int64_t ps, int64_t n_groups, int32_t S, int32_t i0, int32_t i1,
                       int32_t n, const void* L, const double* add, double* tile, double* out, int32_t* st, void* s) {
    return jf::pair_mchain_any<double>(fam, x, xs, p, ps, n_groups, S, i0, i1, n, L, add, tile, out, st, s);
}
int jf_grid_gf_f32(const float* x, int64_t xs, int64_t xgs, const float* p, int64_t ps, int64_t n_groups, int32_t J, int32_t N, int32_t i0, int32_t i1,
                   int32_t D, int32_t n, const jf_gf_layer* L, float* tile, int32_t* st, void* s) {
    return jf::grid_gf<float>(x, xs, xgs, p, ps, n_groups, J, N, i0, i1, D, n, L, tile, st, s);
}
int jf_grid_gf_f64(const double* x, int64_t xs, int64_t xgs, const double* p, int64_t ps, int64_t n_groups, int32_t J, int32_t N, int32_t i0, int32_t i1,
                   int32_t D, int32_t n, const jf_gf_layer* L, double* tile, int32_t* st, void* s) {
    return jf::grid_gf<double>(x, xs, xgs, p, ps, n_groups, J, N, i0, i1, D, n, L, tile, st, s);
}
int jf_grid_mchain_f32(int32_t fam, const float* x, int64_t xs, int64_t xgs, const float* p, int64_t ps, int64_t n_groups, int32_t J, int32_t N,
                       int32_t i0, int32_t i1, int32_t n, const void* L, float* tile, int32_t* st, void* s) {
    return jf::grid_mchain_any<float>(fam, x, xs, xgs, p, ps, n_groups, J, N, i0, i1, n, L, tile, st, s);
}
int jf_grid_mchain_f64(int32_t fam, const double* x, int64_t xs, int64_t xgs, const double* p, int64_t ps, int64_t n_groups, int32_t J, int32_t N,
                       int32_t i0, int32_t i1, int32_t n, const void* L, double* tile, int32_t* st, void* s) {
    return jf::grid_mchain_any<double>(fam, x, xs, xgs, p, ps, n_groups, J, N, i0, i1, n, L, tile, st, s);
}
int jf_grid_reduce_f32(const float* tile, const float* logw, const float* add, int64_t n_groups, int32_t J, int32_t ni, float* out, void* s) {
    return jf::grid_reduce<float>(tile, logw, add, n_groups, J, ni, out, s);
}
int jf_grid_reduce_f64(const double* tile, const double* logw, const double* add, int64_t n_groups, int32_t J, int32_t ni, double* out, void* s) {
    return jf::grid_reduce<double>(tile, logw, add, n_groups, J, ni, out, s);
}
}
