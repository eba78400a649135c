// Density-refined multi-order sky maps (include/jammy_hip_sky_refine.h): per row the K cells that carry the most probability mass, their
// in-order replacement by their four children, and the entropy of the piecewise-constant map.  gfx950, wave64.
//
//   select   ONE workgroup of CHUNK = 256 threads per row.  The key of a cell, (double)lp + logw, is mapped to a uint64 whose unsigned order
//            is the key's order (sign bit flipped for positive keys, all bits for negative ones; -0.0 -> +0.0 and NaN -> -inf first).  Eight
//            passes, most significant byte first: a 256-bin histogram in LDS of the next byte of the keys that share the bytes found so far
//            (integer LDS atomics: the counts do not depend on the order of arrival), a suffix scan of the bins by the workgroup, the bin that
//            holds rank K.  After the last pass the K-th largest key is known exactly, and so is the number of keys equal to it that belong
//            to the result.  One more walk of the row, 256 columns at a time with running counts, places every column: its position is
//            (keys above the threshold before it) + min(keys equal to it before it, those that belong), both from 64-bit ballots and the
//            popcounts of the earlier waves.  No atomic decides a position, nothing depends on C or on the grid.
//            The row is read nine times (from L2 after the first).  One workgroup has four waves to hide the latency of its loads with, so a
//            histogram pass keeps UNROLL = 8 independent loads per thread in flight, with no branch between them -- which is why the presence
//            of log-areas is a template parameter: with a test of the pointer in front of each load a launch at M = 10^6 took 3.3 times as long
//            (DESIGN.md section 14).
//   expand   one thread per input cell: its rank in the row's ascending selection (a binary search) is the number of cells split before it,
//            hence its output column.  No atomics, the nested order is kept by construction.
//            The first K threads of a row also check one entry of the selection each (inside the row, above the entry before it).
//   entropy  one workgroup per row, thread t adds the cells t, t + 256, ... in column order in double, then a fixed tree.
#include "jf_common.h"
#include "jf_sky.h"

#include "../../include/jammy_hip_sky_refine.h"

namespace jf {
namespace sky_refine {

constexpr int CHUNK = JF_SKY_REFINE_CHUNK, WAVES = CHUNK / JF_WAVE, BINS = 256, UNROLL = 8;
constexpr int64_t MAX_ELEMS = ((int64_t)1 << 31) - 1;
static_assert(CHUNK == BINS && CHUNK % JF_WAVE == 0, "one thread per bin, whole waves");

// the order-preserving uint64 image of a key: NaN ranks as -inf, -0.0 as +0.0
__device__ __forceinline__ uint64_t key_image(double key, bool& nan) {
    nan = key != key;
    uint64_t u = (uint64_t)__double_as_longlong(nan ? -INFINITY : key);
    if (u == 0x8000000000000000ull) u = 0;                  // -0.0
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// (W: there are log-areas.  A template parameter, not a test of the pointer: a branch between two loads makes hipcc wait for the first)
template <typename T, bool W>
__device__ __forceinline__ uint64_t image_at(const T* __restrict__ lp, const double* __restrict__ logw, int64_t m, bool& nan) {
    const double v = (double)lp[m];
    if constexpr (W) return key_image(v + logw[m], nan);
    else return key_image(v, nan);
}

template <typename T, bool W>
__global__ void __launch_bounds__(CHUNK) select_kernel(const T* __restrict__ lp, int64_t lp_stride, const double* __restrict__ logw,
                                                       int64_t logw_stride, int64_t M, int64_t K, int64_t* __restrict__ sel_out,
                                                       int32_t* __restrict__ status) {
    __shared__ uint32_t hist[BINS];
    __shared__ uint32_t wave_total[WAVES];
    __shared__ uint32_t found_bin, found_rank;
    __shared__ uint32_t counts[2][2][WAVES];                // [parity of the chunk][above, equal][wave]
    const int tid = threadIdx.x, wave = tid / JF_WAVE, lane = tid % JF_WAVE;
    const T* row = lp + (int64_t)blockIdx.x * lp_stride;
    const double* wrow = logw != nullptr ? logw + (int64_t)blockIdx.x * logw_stride : nullptr;
    int64_t* out = sel_out + (int64_t)blockIdx.x * K;

    // ---- the K-th largest image: prefix = its bytes found so far, rank = its rank (1 = largest) among the keys that share them
    uint64_t prefix = 0;
    uint32_t rank = (uint32_t)K;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for (int64_t base = 0; base < M; base += UNROLL * CHUNK) {
            // UNROLL independent loads per thread and no branch between them: a column past the row re-reads the row's last one, uncounted
            uint64_t u[UNROLL];
            bool in[UNROLL], nan[UNROLL];
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const int64_t m = base + j * CHUNK + tid;
                in[j] = m < M;
                u[j] = image_at<T, W>(row, wrow, in[j] ? m : M - 1, nan[j]);
            }
#pragma unroll
            for (int j = 0; j < UNROLL; ++j) {
                const uint64_t high = pass == 0 ? 0 : u[j] >> (shift + 8);
                if (in[j] && high == prefix) atomicAdd(&hist[(u[j] >> shift) & 0xff], 1u);
                if (pass == 0) status_add(status, JF_STATUS_NONFINITE, in[j] && nan[j], (unsigned)lane);
            }
        }
        __syncthreads();
        // bins in descending order, one per thread: inclusive scan over the workgroup
        const uint32_t v = hist[BINS - 1 - tid];
        uint32_t incl = v;
#pragma unroll
        for (int off = 1; off < JF_WAVE; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, JF_WAVE);
            if (lane >= off) incl += up;
        }
        if (lane == JF_WAVE - 1) wave_total[wave] = incl;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < WAVES; ++k) incl += k < wave ? wave_total[k] : 0;
        if (incl >= rank && incl - v < rank) {              // exactly one thread: the counts of the bins ascend to at least `rank`
            found_bin = (uint32_t)(BINS - 1 - tid);
            found_rank = rank - (incl - v);
        }
        __syncthreads();
        prefix = (prefix << 8) | found_bin;
        rank = found_rank;
    }
    // prefix = the K-th largest image; `rank` of the keys equal to it belong to the result: the first ones by column

    // ---- the ordered walk
    uint32_t run_above = 0, run_equal = 0;
    int par = 0;
    for (int64_t base = 0; base < M; base += CHUNK, par ^= 1) {
        const int64_t m = base + tid;
        bool above = false, equal = false, nan = false;
        if (m < M) {
            const uint64_t u = image_at<T, W>(row, wrow, m, nan);
            above = u > prefix;
            equal = u == prefix;
        }
        const unsigned long long word_above = __ballot(above), word_equal = __ballot(equal);
        if (lane == 0) {
            counts[par][0][wave] = (uint32_t)__popcll(word_above);
            counts[par][1][wave] = (uint32_t)__popcll(word_equal);
        }
        __syncthreads();                                    // (the other parity is written next: a wave may run one chunk ahead, not two)
        const unsigned long long below_lane = (1ull << lane) - 1ull;
        uint32_t above_before = (uint32_t)__popcll(word_above & below_lane), equal_before = (uint32_t)__popcll(word_equal & below_lane);
        uint32_t chunk_above = 0, chunk_equal = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) {
            const uint32_t a = counts[par][0][k], e = counts[par][1][k];
            above_before += k < wave ? a : 0;
            equal_before += k < wave ? e : 0;
            chunk_above += a;
            chunk_equal += e;
        }
        const uint32_t equal_rank = run_equal + equal_before;
        const int64_t pos = (int64_t)(run_above + above_before) + (int64_t)(equal_rank < rank ? equal_rank : rank);
        if ((above || (equal && equal_rank < rank)) && pos < K) out[pos] = m;
        run_above += chunk_above;
        run_equal += chunk_equal;
    }
}

template <typename T>
__global__ void __launch_bounds__(CHUNK) expand_kernel(const int64_t* __restrict__ uniq_in, const T* __restrict__ lp_in,
                                                       const int64_t* __restrict__ sel, int64_t C, int64_t M, int64_t K,
                                                       int64_t* __restrict__ uniq_out, T* __restrict__ lp_out, int64_t* __restrict__ new_cols,
                                                       int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
    bool stuck = false;
    if (i < C * M) {
        const int64_t c = i / M, m = i - c * M;
        const int64_t* srow = sel + c * K;
        const int64_t r = sky::lower_bound(srow, K, m);     // selected columns below m: r <= K, so every index below stays inside its row
        const int64_t col = m + 3 * r, Mo = M + 3 * K;
        // the first K threads of a row also check one entry of its selection each: inside [0, M) and above the entry before it.  A row whose
        // selection breaks the contract is counted, entry by entry; its output columns are then not all written
        if (m < K) stuck = srow[m] < 0 || srow[m] >= M || (m > 0 && srow[m - 1] >= srow[m]);
        const int64_t u = uniq_in[i];
        int64_t* uo = uniq_out + c * Mo + col;
        T* lo = lp_out + c * Mo + col;
        if (r < K && srow[r] == m) {
            int order = 0;
            int64_t pix = 0;
            const bool split = sky::decode_uniq(u, order, pix) && order < sky::MAX_ORDER;
            stuck = stuck || !split;
            int64_t* nc = new_cols + c * 4 * K + 4 * r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uo[j] = split ? 4 * u + j : (j == 0 ? u : (int64_t)-1);
                lo[j] = split ? (T)NAN : (j == 0 ? lp_in[i] : (T)-INFINITY);
                nc[j] = split ? col + j : (int64_t)-1;
            }
        } else {
            uo[0] = u;
            lo[0] = lp_in[i];
        }
    }
    status_add(status, JF_STATUS_OUT_OF_RANGE, stuck);
}

template <typename T>
__global__ void __launch_bounds__(CHUNK) entropy_kernel(const T* __restrict__ lp, int64_t lp_stride, const double* __restrict__ logw,
                                                        int64_t logw_stride, int64_t M, const double* __restrict__ log_norm,
                                                        double* __restrict__ entropy) {
    __shared__ double wave_part[WAVES];
    const int tid = threadIdx.x, wave = tid / JF_WAVE, lane = tid % JF_WAVE;
    const T* row = lp + (int64_t)blockIdx.x * lp_stride;
    const double* wrow = logw != nullptr ? logw + (int64_t)blockIdx.x * logw_stride : nullptr;
    const double ln = log_norm[blockIdx.x];
    double acc = 0.0;
    for (int64_t m = tid; m < M; m += CHUNK) {
        const double v = (double)row[m];
        const double a = wrow != nullptr ? v + wrow[m] : v;
        if (v != -INFINITY) acc += exp(a - ln) * v;         // (exp(-inf) * -inf would be NaN: an empty cell contributes 0)
    }
    acc = wave_sum(acc);                                    // the butterfly's order is fixed
    if (lane == 0) wave_part[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) s += wave_part[k];
        entropy[blockIdx.x] = ln - s;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
static unsigned blocks_of(int64_t n) { return (unsigned)((n + CHUNK - 1) / CHUNK); }

static bool logw_ok(const double* logw, int64_t logw_stride, int64_t M) {
    return logw == nullptr || logw_stride == 0 || logw_stride >= M;
}

template <typename T>
static int select(const T* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M, int64_t K, int64_t* sel_out,
                  int32_t* status, void* stream) {
    if (!lp || !sel_out || C < 0 || M < 0 || K < 0 || K > M || lp_stride < M || !logw_ok(logw, logw_stride, M)) return JF_ERR_BADARG;
    int64_t n = 0;
    if (__builtin_mul_overflow(C, M, &n) || n > MAX_ELEMS) return JF_ERR_UNSUPPORTED;
    if (C == 0 || K == 0) return JF_OK;
    if (logw != nullptr)
        jf::launch(select_kernel<T, true>, dim3((unsigned)C), dim3(CHUNK), 0, (hipStream_t)stream, lp, lp_stride, logw, logw_stride, M, K, sel_out,
                   status);
    else
        jf::launch(select_kernel<T, false>, dim3((unsigned)C), dim3(CHUNK), 0, (hipStream_t)stream, lp, lp_stride, logw, logw_stride, M, K, sel_out,
                   status);
    return check_launch();
}

template <typename T>
static int expand(const int64_t* uniq_in, const T* lp_in, const int64_t* sel, int64_t C, int64_t M, int64_t K, int64_t* uniq_out, T* lp_out,
                  int64_t* new_cols, int32_t* status, void* stream) {
    if (!uniq_in || !lp_in || !uniq_out || !lp_out || C < 0 || M < 0 || K < 0 || K > M) return JF_ERR_BADARG;
    if (K > 0 && (!sel || !new_cols)) return JF_ERR_BADARG;
    int64_t n = 0;
    if (M > MAX_ELEMS || __builtin_mul_overflow(C, M + 3 * K, &n) || n > MAX_ELEMS) return JF_ERR_UNSUPPORTED;
    if (C == 0 || M == 0) return JF_OK;
    jf::launch(expand_kernel<T>, dim3(blocks_of(C * M)), dim3(CHUNK), 0, (hipStream_t)stream, uniq_in, lp_in, sel, C, M, K, uniq_out, lp_out,
               new_cols, status);
    return check_launch();
}

template <typename T>
static int entropy(const T* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M, const double* log_norm,
                   double* entropy_out, void* stream) {
    if (!lp || !log_norm || !entropy_out || C < 0 || M < 0 || lp_stride < M || !logw_ok(logw, logw_stride, M)) return JF_ERR_BADARG;
    int64_t n = 0;
    if (__builtin_mul_overflow(C, M, &n) || n > MAX_ELEMS) return JF_ERR_UNSUPPORTED;
    if (C == 0 || M == 0) return JF_OK;
    jf::launch(entropy_kernel<T>, dim3((unsigned)C), dim3(CHUNK), 0, (hipStream_t)stream, lp, lp_stride, logw, logw_stride, M, log_norm,
               entropy_out);
    return check_launch();
}

}  // namespace sky_refine
}  // namespace jf

extern "C" {
int jf_sky_refine_abi_version(void) { return 1; }
#define JF_SKY_REFINE_ENTRY(T, SUF)                                                                                                          \
    int jf_sky_refine_select_##SUF(const T* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M, int64_t K,   \
                                   int64_t* sel_out, int32_t* status, void* s) {                                                             \
        return jf::sky_refine::select<T>(lp, lp_stride, logw, logw_stride, C, M, K, sel_out, status, s);                                     \
    }                                                                                                                                        \
    int jf_sky_refine_expand_##SUF(const int64_t* uniq_in, const T* lp_in, const int64_t* sel, int64_t C, int64_t M, int64_t K,                \
                                   int64_t* uniq_out, T* lp_out, int64_t* new_cols, int32_t* status, void* s) {                              \
        return jf::sky_refine::expand<T>(uniq_in, lp_in, sel, C, M, K, uniq_out, lp_out, new_cols, status, s);                               \
    }                                                                                                                                        \
    int jf_sky_refine_entropy_##SUF(const T* lp, int64_t lp_stride, const double* logw, int64_t logw_stride, int64_t C, int64_t M,             \
                                    const double* log_norm, double* entropy, void* s) {                                                      \
        return jf::sky_refine::entropy<T>(lp, lp_stride, logw, logw_stride, C, M, log_norm, entropy, s);                                     \
    }
JF_SKY_REFINE_ENTRY(float, f32)
JF_SKY_REFINE_ENTRY(double, f64)
#undef JF_SKY_REFINE_ENTRY
}
