// Segmented order statistics (include/jammy_hip_order.h): sort every column of many short segments, then read quantiles and shortest
// intervals off the sorted rows.  gfx950, wave64.
//
//   sort       ONE workgroup per (segment, column).  The S values are mapped to integer keys of their own width whose unsigned order is the
//              order of the header (one to one, so the sorted values are recovered from the sorted keys bit for bit and nothing but keys is
//              held), S keys in dynamic LDS -- sized to the segment, so that short segments share a CU: 4 KB at S = 1000 in float32, 128 KiB
//              at the cap in float64, which takes the opt-in of jf_common.h.  A bitonic network in the form whose every exchange moves the
//              smaller key to the LOWER index: the first step of a merge of width k pairs i with i ^ (k - 1), the later ones i with i + j.
//              Positions S .. P - 1 of the power of two P >= S then behave as keys above every key -- an exchange with one of them is no
//              exchange -- so they are neither stored nor visited: no padding key is needed (the keys use every value of their width) and
//              S is arbitrary.
//              LDS access: pair t of a step of distance j touches lo = 2 j (t / j) + t % j and its partner.  For j >= 32 (float32) or j >= 16
//              (float64) the 32 lanes of a half-wave read consecutive keys: no bank conflict.  Below that the lanes' addresses spread over
//              2 j-key blocks with a gap: 2-way conflicts in log2(32) of the log2(P) steps of a merge; the workgroup's barrier per step, not
//              the LDS, bounds a step.
//              256 threads up to P = 4096, 1024 above: at least two pairs per thread and step where the segment has them.
//              The column read is strided (x_stride elements between the entries of a column) and the W workgroups of a segment read the
//              same S * x_stride elements: the first takes them from HBM, the others from L2.
//   quantiles  one thread per (row, probability): two loads and one interpolation in double.
//   shortest   one workgroup of 256 threads per row; per count, thread t scans the starts t, t + 256, ... in ascending order and keeps the
//              first least (width, i); a fixed butterfly over the wave and a fixed loop over the four waves reduce the pairs.  The order of
//              (width, i) pairs is total, so the result does not depend on the tree; it is fixed all the same.
#include "jf_common.h"

#include "../../include/jammy_hip_order.h"

namespace jf {
namespace order {

constexpr int SMALL = 256, LARGE = 1024, ROW = 256;
constexpr int64_t MAX_ELEMS = ((int64_t)1 << 31) - 1;

template <typename T> struct Key;
template <> struct Key<float> {
    using U = uint32_t;
    static constexpr U SIGN = 0x80000000u, MANT = 0x007fffffu, EXPO = 0x7f800000u;
    static __device__ __forceinline__ U bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float value(U u) { return __uint_as_float(u); }
};
template <> struct Key<double> {
    using U = uint64_t;
    static constexpr U SIGN = 0x8000000000000000ull, MANT = 0x000fffffffffffffull, EXPO = 0x7ff0000000000000ull;
    static __device__ __forceinline__ U bits(double v) { return (U)__double_as_longlong(v); }
    static __device__ __forceinline__ double value(U u) { return __longlong_as_double((long long)u); }
};

// the key of the header: numbers from 0 (-inf) to 2 EXPO + 1 (+inf), NaNs above by payload, then sign
template <typename T> __device__ __forceinline__ typename Key<T>::U key_of(T v, bool& nan) {
    using K = Key<T>;
    using U = typename K::U;
    const U u = K::bits(v), mant = u & K::MANT;
    nan = (u & K::EXPO) == K::EXPO && mant != 0;
    if (nan) return (U)(2 * K::EXPO + 2) + 2 * (mant - 1) + (u >> (8 * sizeof(U) - 1));
    return ((u & K::SIGN) ? ~u : (u | K::SIGN)) - K::MANT;
}

template <typename T> __device__ __forceinline__ bool key_is_nan(typename Key<T>::U k) { return k > 2 * Key<T>::EXPO + 1; }

template <typename T> __device__ __forceinline__ T value_of(typename Key<T>::U k) {
    using K = Key<T>;
    using U = typename K::U;
    if (key_is_nan<T>(k)) {
        const U r = k - (U)(2 * K::EXPO + 2);
        return K::value(((r & 1) ? K::SIGN : (U)0) | K::EXPO | ((r >> 1) + 1));
    }
    const U image = k + K::MANT;
    return K::value((image & K::SIGN) ? (image ^ K::SIGN) : ~image);
}

template <typename T, int THREADS>
__global__ void __launch_bounds__(THREADS) sort_kernel(const T* __restrict__ x, int64_t x_stride, int S, int W, int P, T* __restrict__ sorted_out,
                                                       int64_t* __restrict__ n_valid_out, int32_t* __restrict__ status) {
    using U = typename Key<T>::U;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    U* keys = reinterpret_cast<U*>(lds_raw);
    const int tid = threadIdx.x;
    const int64_t gw = blockIdx.x, g = gw / W, w = gw - g * W;
    const T* col = x + g * S * x_stride + w;

    for (int base = 0; base < S; base += THREADS) {          // (whole waves walk the loop: the ballot of status_add sees every lane)
        const int s = base + tid;
        bool nan = false;
        if (s < S) keys[s] = key_of<T>(col[(int64_t)s * x_stride], nan);
        status_add(status, JF_STATUS_NONFINITE, nan);
    }
    __syncthreads();

    const int pairs = P >> 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const bool flip = j == (k >> 1);
            for (int t = tid; t < pairs; t += THREADS) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = flip ? (lo ^ (k - 1)) : (lo + j);
                if (hi < S) {                                 // (lo < hi; a partner at or past S stands for a key above every key)
                    const U a = keys[lo], b = keys[hi];
                    if (b < a) {
                        keys[lo] = b;
                        keys[hi] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

    T* out = sorted_out + gw * S;
    for (int s = tid; s < S; s += THREADS) {
        const U k = keys[s];
        out[s] = value_of<T>(k);
        // the first NaN key, or the end of the row, ends the numbers: exactly one thread sees the boundary
        const bool is_nan = key_is_nan<T>(k);
        if (!is_nan && (s + 1 == S || key_is_nan<T>(keys[s + 1]))) n_valid_out[gw] = s + 1;
        if (is_nan && s == 0) n_valid_out[gw] = 0;
    }
}

template <typename T>
__global__ void __launch_bounds__(ROW) quantiles_kernel(const T* __restrict__ sorted, const int64_t* __restrict__ n_valid, int64_t R, int64_t S,
                                                        const double* __restrict__ probs, int64_t Q, T* __restrict__ out,
                                                        int32_t* __restrict__ status) {
    const int64_t idx = (int64_t)blockIdx.x * ROW + threadIdx.x;
    bool outside = false;
    if (idx < R * Q) {
        const int64_t r = idx / Q, q = idx - r * Q;
        int64_t n = n_valid != nullptr ? n_valid[r] : S;
        n = n < 0 ? 0 : (n > S ? S : n);
        const double p = probs[q];
        outside = !(p >= 0.0 && p <= 1.0);
        T res = (T)NAN;
        if (!outside && n > 0) {
            const T* row = sorted + r * S;
            // (h is the ROUNDED product: fused into h - floor(h) the product would keep bits below h's last place, and a whole rank, t == 0,
            // would be missed)
            double h = p * (double)(n - 1);
            asm volatile("" : "+v"(h));
            const double fl = floor(h);
            const int64_t i = (int64_t)fl;
            const double t = h - fl;
            const double a = (double)row[i];
            if (t == 0.0) {
                res = row[i];
            } else {
                const double b = (double)row[i + 1 < n ? i + 1 : n - 1];
                // the product stays a rounded double of its own: fused into the addition it keeps bits that a host restatement of the rule
                // cannot have, and where a and b differ in sign the result then differs by several of ITS ulps (4 were seen)
                double step = t * (b - a);
                asm volatile("" : "+v"(step));
                res = (T)(a + step);
            }
        }
        out[idx] = res;
    }
    status_add(status, JF_STATUS_OUT_OF_RANGE, outside);
}

// (width, i) pairs: the smaller width first, equal widths to the lower start
__device__ __forceinline__ bool pair_less(double wa, int ia, double wb, int ib) { return wa < wb || (wa == wb && ia < ib); }

template <typename T>
__global__ void __launch_bounds__(ROW) shortest_kernel(const T* __restrict__ sorted, const int64_t* __restrict__ n_valid, int64_t S,
                                                       const int64_t* __restrict__ counts, int64_t T_counts, double period,
                                                       T* __restrict__ low, T* __restrict__ high, double* __restrict__ width,
                                                       int64_t* __restrict__ start, int32_t* __restrict__ status) {
    constexpr int WAVES = ROW / JF_WAVE;
    __shared__ double wave_w[WAVES];
    __shared__ int wave_i[WAVES];
    const int tid = threadIdx.x, wave = tid / JF_WAVE, lane = tid % JF_WAVE;
    const int64_t r = blockIdx.x;
    const T* row = sorted + r * S;
    int64_t n64 = n_valid != nullptr ? n_valid[r] : S;
    n64 = n64 < 0 ? 0 : (n64 > S ? S : n64);
    const int n = (int)n64;
    const bool circular = period > 0.0;

    for (int64_t t = 0; t < T_counts; ++t) {
        const int64_t o = r * T_counts + t;
        if (n == 0) {                                        // (uniform over the workgroup)
            if (tid == 0) {
                low[o] = (T)NAN;
                high[o] = (T)NAN;
                width[o] = (double)NAN;
                if (start != nullptr) start[o] = -1;
            }
            continue;
        }
        int64_t k64 = counts[t];
        k64 = k64 < 1 ? 1 : (k64 > n ? n : k64);
        const int k = (int)k64;
        const int n_starts = circular ? n : n - k + 1;
        double best_w = INFINITY;
        int best_i = 0x7fffffff;
        for (int i = tid; i < n_starts; i += ROW) {
            const int j = i + k - 1;
            double wd = (double)row[j >= n ? j - n : j] - (double)row[i];
            if (j >= n) wd += period;
            wd = wd != wd ? INFINITY : wd;
            if (pair_less(wd, i, best_w, best_i)) {
                best_w = wd;
                best_i = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ow = __shfl_xor(best_w, off, JF_WAVE);
            const int oi = __shfl_xor(best_i, off, JF_WAVE);
            if (pair_less(ow, oi, best_w, best_i)) {
                best_w = ow;
                best_i = oi;
            }
        }
        if (lane == 0) {
            wave_w[wave] = best_w;
            wave_i[wave] = best_i;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int v = 1; v < WAVES; ++v)
                if (pair_less(wave_w[v], wave_i[v], best_w, best_i)) {
                    best_w = wave_w[v];
                    best_i = wave_i[v];
                }
            const int i = best_i, j = i + k - 1;             // (start 0 always stands: best_i is a start of this row)
            const T a = row[i], b = row[j >= n ? j - n : j];
            double wd = (double)b - (double)a;
            if (j >= n) wd += period;
            low[o] = a;
            high[o] = b;
            width[o] = wd;
            if (start != nullptr) start[o] = i;
            if (status != nullptr && !(fabs(wd) < INFINITY)) atomicAdd(status + JF_STATUS_NONFINITE, 1);
        }
        __syncthreads();                                     // (wave_w / wave_i are written again for the next count)
    }
}

// ------------------------------------------------------------------------------------------------------------ host
static bool tile_ok(int64_t a, int64_t b) {
    int64_t n = 0;
    return !__builtin_mul_overflow(a, b, &n) && n <= MAX_ELEMS;
}

template <typename T>
static int sort(const T* x, int64_t x_stride, int64_t G, int64_t S, int64_t W, T* sorted_out, int64_t* n_valid_out, int32_t* status,
                void* stream) {
    if (!x || !sorted_out || !n_valid_out || G < 0 || S < 0 || W < 0 || x_stride < W) return JF_ERR_BADARG;
    int64_t gw = 0, n = 0;
    if (S > JF_ORDER_MAX_S || __builtin_mul_overflow(G, W, &gw) || __builtin_mul_overflow(gw, S, &n) || n > MAX_ELEMS || gw > MAX_ELEMS)
        return JF_ERR_UNSUPPORTED;
    if (G == 0 || S == 0 || W == 0) return JF_OK;
    int P = 1;
    while (P < S) P <<= 1;
    const size_t lds = (size_t)S * sizeof(typename Key<T>::U);
    if (P <= 4 * LARGE) {
        allow_lds(sort_kernel<T, SMALL>, lds);
        jf::launch(sort_kernel<T, SMALL>, dim3((unsigned)gw), dim3(SMALL), lds, (hipStream_t)stream, x, x_stride, (int)S, (int)W, P, sorted_out,
                   n_valid_out, status);
    } else {
        allow_lds(sort_kernel<T, LARGE>, lds);
        jf::launch(sort_kernel<T, LARGE>, dim3((unsigned)gw), dim3(LARGE), lds, (hipStream_t)stream, x, x_stride, (int)S, (int)W, P, sorted_out,
                   n_valid_out, status);
    }
    return check_launch();
}

template <typename T>
static int quantiles(const T* sorted, const int64_t* n_valid, int64_t R, int64_t S, const double* probs, int64_t Q, T* out, int32_t* status,
                     void* stream) {
    if (!sorted || !probs || !out || R < 0 || S < 0 || Q < 0) return JF_ERR_BADARG;
    if (!tile_ok(R, S) || !tile_ok(R, Q)) return JF_ERR_UNSUPPORTED;
    if (R == 0 || S == 0 || Q == 0) return JF_OK;
    jf::launch(quantiles_kernel<T>, dim3((unsigned)((R * Q + ROW - 1) / ROW)), dim3(ROW), 0, (hipStream_t)stream, sorted, n_valid, R, S, probs, Q,
               out, status);
    return check_launch();
}

template <typename T>
static int shortest(const T* sorted, const int64_t* n_valid, int64_t R, int64_t S, const int64_t* counts, int64_t Tn, double period, T* low,
                    T* high, double* width, int64_t* start, int32_t* status, void* stream) {
    if (!sorted || !counts || !low || !high || !width || R < 0 || S < 0 || Tn < 0) return JF_ERR_BADARG;
    if (!tile_ok(R, S) || !tile_ok(R, Tn)) return JF_ERR_UNSUPPORTED;
    if (R == 0 || S == 0 || Tn == 0) return JF_OK;
    jf::launch(shortest_kernel<T>, dim3((unsigned)R), dim3(ROW), 0, (hipStream_t)stream, sorted, n_valid, S, counts, Tn, period, low, high, width,
               start, status);
    return check_launch();
}

}  // namespace order
}  // namespace jf

extern "C" {
int jf_order_abi_version(void) { return 1; }
#define JF_ORDER_ENTRY(T, SUF)                                                                                                               \
    int jf_order_sort_##SUF(const T* x, int64_t x_stride, int64_t G, int64_t S, int64_t W, T* sorted_out, int64_t* n_valid_out,              \
                            int32_t* status, void* s) {                                                                                      \
        return jf::order::sort<T>(x, x_stride, G, S, W, sorted_out, n_valid_out, status, s);                                                 \
    }                                                                                                                                        \
    int jf_order_quantiles_##SUF(const T* sorted, const int64_t* n_valid, int64_t R, int64_t S, const double* probs, int64_t Q, T* out,     \
                                 int32_t* status, void* s) {                                                                                 \
        return jf::order::quantiles<T>(sorted, n_valid, R, S, probs, Q, out, status, s);                                                    \
    }                                                                                                                                        \
    int jf_order_shortest_##SUF(const T* sorted, const int64_t* n_valid, int64_t R, int64_t S, const int64_t* counts, int64_t T_counts,     \
                                double period, T* low, T* high, double* width, int64_t* start, int32_t* status, void* s) {                   \
        return jf::order::shortest<T>(sorted, n_valid, R, S, counts, T_counts, period, low, high, width, start, status, s);                  \
    }
JF_ORDER_ENTRY(float, f32)
JF_ORDER_ENTRY(double, f64)
#undef JF_ORDER_ENTRY
}
