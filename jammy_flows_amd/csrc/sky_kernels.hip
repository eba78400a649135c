// Sky maps (include/jammy_hip_sky.h): the HEALPix pixelisation of the sphere in the NESTED scheme (Gorski et al. 2005, ApJ 622, 759, section 4
// and appendix), and the counting / locating steps of an adaptive multi-order mesh -- what the reference does on the host with healpy and
// mhealpy (helper_fns/plotting/spherical.py:452-549).  gfx950, wave64.
//
// Every kernel is one thread per element (direction, cell or pixel), reads a few words, does some tens of double / int64 operations and
// writes one row: they are launch- and latency-bound at the sizes a mesh has (10^4 .. 10^7 elements), and there is nothing to stage or
// share between threads.  All arithmetic is double and int64 for both tile types, so a pixel index does not depend on the input's type.
//
// A direction's pixel is computed once at order 29 (nside 2^29, indices below 12 * 2^58) and shifted right by 2 * (29 - order): the
// nestedness pix(o) == pix(29) >> 2 (29 - o) then holds by construction instead of by the luck of two roundings.  A cell of order o covers
// the order-29 indices [pix << 2 (29 - o), (pix + 1) << 2 (29 - o)), which is what counting and locating work on.
//
// The reductions of the header (jf_sky_hpd_*, jf_sky_region_volume_*) are the kernels of hpd_kernels.hip and live there.
#include "jf_common.h"
#include "jf_sky.h"          // decode_uniq, lower_bound, MAX_ORDER

namespace jf {
namespace sky {

constexpr int THREADS = 256;
constexpr int64_t NS29 = (int64_t)1 << MAX_ORDER;
constexpr double PI = 3.141592653589793238462643383279502884, HALF_PI = 0.5 * PI, TWO_OVER_PI = 2.0 / PI, TWO_THIRDS = 2.0 / 3.0;

// bits 0..31 of v onto the even bits of the result
__host__ __device__ __forceinline__ uint64_t spread_bits(uint64_t v) {
    v &= 0xffffffffull;
    v = (v | (v << 16)) & 0x0000ffff0000ffffull;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}
// ... and back: the even bits of v, packed
__host__ __device__ __forceinline__ uint64_t compress_bits(uint64_t v) {
    v &= 0x5555555555555555ull;
    v = (v | (v >> 1)) & 0x3333333333333333ull;
    v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v >> 4)) & 0x00ff00ff00ff00ffull;
    v = (v | (v >> 8)) & 0x0000ffff0000ffffull;
    v = (v | (v >> 16)) & 0x00000000ffffffffull;
    return v;
}

// the order-29 nested pixel of a direction given as z = cos(theta), rho2 = sin^2(theta) = 1 - z^2 (passed separately: near the poles it is
// known to full relative precision while 1 - |z| computed from z is not) and the azimuth phi (any finite value)
__host__ __device__ __forceinline__ int64_t ang2pix29(double z, double rho2, double phi) {
    const double za = fabs(z);
    double tt = phi * TWO_OVER_PI;                         // in [0, 4)
    tt -= 4.0 * floor(tt * 0.25);
    if (!(tt < 4.0)) tt = 0.0;
    if (tt < 0.0) tt = 0.0;
    const double ns = (double)NS29;
    int64_t face, ix, iy;
    if (za <= TWO_THIRDS) {                                // equatorial belt
        const double t1 = ns * (0.5 + tt), t2 = ns * z * 0.75;
        const int64_t jp = (int64_t)floor(t1 - t2);        // index of the ascending edge line
        const int64_t jm = (int64_t)floor(t1 + t2);        // ... of the descending one
        const int64_t ifp = jp >> MAX_ORDER, ifm = jm >> MAX_ORDER;
        face = ifp == ifm ? (ifp & 3) + 4 : (ifp < ifm ? (ifp & 3) : (ifm & 3) + 8);
        ix = jm & (NS29 - 1);
        iy = NS29 - (jp & (NS29 - 1)) - 1;
    } else {                                               // polar caps
        int64_t ntt = (int64_t)tt;
        if (ntt > 3) ntt = 3;
        const double tp = tt - (double)ntt;
        const double omza = rho2 / (1.0 + za);             // 1 - |z|
        const double tmp = ns * sqrt(3.0 * omza);
        int64_t jp = (int64_t)(tp * tmp), jm = (int64_t)((1.0 - tp) * tmp);
        if (jp > NS29 - 1) jp = NS29 - 1;
        if (jm > NS29 - 1) jm = NS29 - 1;
        if (z >= 0.0) { face = ntt; ix = NS29 - jm - 1; iy = NS29 - jp - 1; }
        else { face = ntt + 8; ix = jp; iy = jm; }
    }
    return (face << (2 * MAX_ORDER)) + (int64_t)(spread_bits((uint64_t)ix) | (spread_bits((uint64_t)iy) << 1));
}

template <typename T>
__global__ void __launch_bounds__(THREADS) vec2pix_kernel(const T* __restrict__ v, int64_t stride, int32_t ncol, int64_t B, int32_t order,
                                                          int64_t* __restrict__ pix_out, int32_t* __restrict__ status) {
    const int64_t b = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool active = b < B;
    bool bad = false;
    int64_t pix = -1;
    if (active) {
        const T* row = v + b * stride;
        double z, rho2, phi;
        if (ncol == 3) {
            const double x = (double)row[0], y = (double)row[1], zz = (double)row[2];
            // scaled by the largest component, so that neither the squares of a long vector overflow nor those of a short one vanish
            const double s = fmax(fabs(x), fmax(fabs(y), fabs(zz)));
            const double xs = x / s, ys = y / s, zs = zz / s;
            const double xy2 = xs * xs + ys * ys, r2 = xy2 + zs * zs;
            bad = !(s > 0.0) || !(s < INFINITY) || !(r2 >= 1.0 && r2 <= 3.0);      // (fmax skips a NaN component; r2 does not)
            z = zs / sqrt(r2);
            rho2 = xy2 / r2;
            phi = atan2(y, x);
        } else {
            // (a float pi, 3.14159274, lies above the double one: zeniths up to it are the south pole's)
            const double theta = fmin((double)row[0], PI);
            phi = (double)row[1];
            bad = !(theta >= 0.0 && (double)row[0] <= 3.1415927410125732) || !(fabs(phi) < INFINITY);
            const double st = sin(theta);
            z = cos(theta);
            rho2 = st * st;
        }
        if (!bad) pix = ang2pix29(z, rho2, phi) >> (2 * (MAX_ORDER - order));
        pix_out[b] = pix;
    }
    status_add(status, JF_STATUS_NONFINITE, active && bad);
}

// centre of nested pixel `pix` at `order`: z = cos(theta), sth = sin(theta) and the azimuth.  The face tables of the paper,
// jrll = {2,2,2,2, 3,3,3,3, 4,4,4,4} and jpll = {1,3,5,7, 0,2,4,6, 1,3,5,7}, are 2 + face / 4 and 2 (face % 4) + (face / 4 != 1).
__host__ __device__ __forceinline__ void pix2loc(int order, int64_t pix, double& z, double& sth, double& phi) {
    const int64_t ns = (int64_t)1 << order;
    const int face = (int)(pix >> (2 * order));
    const uint64_t in_face = (uint64_t)(pix & ((ns * ns) - 1));
    const int64_t ix = (int64_t)compress_bits(in_face), iy = (int64_t)compress_bits(in_face >> 1);
    const int64_t jrll = 2 + (face >> 2), jpll = 2 * (face & 3) + ((face >> 2) != 1 ? 1 : 0);
    const int64_t jr = jrll * ns - ix - iy - 1;            // ring, counted from the north pole (1 .. 4 ns - 1)
    const double dns = (double)ns;
    int64_t nr;
    if (jr < ns) {                                         // north cap: 1 - z = nr^2 / (3 ns^2), known exactly where z itself rounds to 1
        nr = jr;
        const double omz = ((double)nr * (double)nr) / (3.0 * dns * dns);
        z = 1.0 - omz;
        sth = sqrt(omz * (2.0 - omz));
    } else if (jr > 3 * ns) {                              // south cap
        nr = 4 * ns - jr;
        const double omz = ((double)nr * (double)nr) / (3.0 * dns * dns);
        z = omz - 1.0;
        sth = sqrt(omz * (2.0 - omz));
    } else {                                               // equatorial belt
        nr = ns;
        z = (double)(2 * ns - jr) * 2.0 / (3.0 * dns);
        sth = sqrt((1.0 - z) * (1.0 + z));
    }
    // phi = (jp - (ks + 1) / 2) (pi / 2) / nr with jp = (jpll nr + ix - iy + 1 + ks) / 2: the ring shift ks cancels
    int64_t t = jpll * nr + ix - iy;
    if (t < 0) t += 8 * nr;
    phi = (double)t * (0.5 * HALF_PI) / (double)nr;
}

template <typename T>
__global__ void __launch_bounds__(THREADS) cell_centres_kernel(const int64_t* __restrict__ uniq, int64_t M, int32_t ncol, T* __restrict__ out,
                                                               int64_t stride) {
    const int64_t m = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    int order = 0;
    int64_t pix = 0;
    double z = 1.0, sth = 0.0, phi = 0.0;                  // padding: the north pole
    if (decode_uniq(uniq[m], order, pix)) pix2loc(order, pix, z, sth, phi);
    T* row = out + m * stride;
    if (ncol == 3) {
        row[0] = (T)(sth * cos(phi));
        row[1] = (T)(sth * sin(phi));
        row[2] = (T)z;
    } else {
        row[0] = (T)atan2(sth, z);
        row[1] = (T)phi;
    }
}

__global__ void __launch_bounds__(THREADS) cell_counts_kernel(const int64_t* __restrict__ sorted_pix, int64_t stride, int64_t G, int64_t S,
                                                              const int64_t* __restrict__ uniq, const int64_t* __restrict__ row_of_cell,
                                                              int64_t n_cells, int64_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_cells) return;
    int order = 0;
    int64_t pix = 0, n = 0;
    const int64_t g = row_of_cell[i];
    if (g >= 0 && g < G && decode_uniq(uniq[i], order, pix)) {
        const int sh = 2 * (MAX_ORDER - order);
        const int64_t* row = sorted_pix + g * stride;
        const int64_t first = lower_bound(row, S, pix << sh);
        n = lower_bound(row, S, (pix + 1) << sh) - first;
    }
    counts[i] = n;
}

__global__ void __launch_bounds__(THREADS) locate_kernel(const int64_t* __restrict__ cell_start, const int64_t* __restrict__ offsets, int64_t G,
                                                         const int64_t* __restrict__ pix, int64_t T, int64_t* __restrict__ cell_out) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= G * T) return;
    const int64_t g = i / T, p = pix[i];
    const int64_t a = offsets[g], b = offsets[g + 1];
    int64_t cell = -1;
    if (p >= 0 && b > a && a >= 0) cell = a + lower_bound(cell_start + a, b - a, p + 1) - 1;     // upper_bound - 1
    cell_out[i] = cell < a ? -1 : cell;
}

// ------------------------------------------------------------------------------------------------------------ host
constexpr int64_t MAX_ELEMS = ((int64_t)1 << 31) - 1;      // elements of one launch: grid.x = ceil(n / THREADS) stays far below 2^31

static unsigned blocks_of(int64_t n) { return (unsigned)((n + THREADS - 1) / THREADS); }

template <typename T>
static int vec2pix(const T* v, int64_t stride, int32_t ncol, int64_t B, int32_t order, int64_t* pix_out, int32_t* status, void* stream) {
    if (!v || !pix_out || B < 0 || (ncol != 2 && ncol != 3) || stride < ncol || order < 0 || order > MAX_ORDER) return JF_ERR_BADARG;
    if (B > MAX_ELEMS) return JF_ERR_UNSUPPORTED;
    if (B == 0) return JF_OK;
    jf::launch(vec2pix_kernel<T>, dim3(blocks_of(B)), dim3(THREADS), 0, (hipStream_t)stream, v, stride, ncol, B, order, pix_out, status);
    return check_launch();
}

template <typename T> static int cell_centres(const int64_t* uniq, int64_t M, int32_t ncol, T* out, int64_t stride, void* stream) {
    if (!uniq || !out || M < 0 || (ncol != 2 && ncol != 3) || stride < ncol) return JF_ERR_BADARG;
    if (M > MAX_ELEMS) return JF_ERR_UNSUPPORTED;
    if (M == 0) return JF_OK;
    jf::launch(cell_centres_kernel<T>, dim3(blocks_of(M)), dim3(THREADS), 0, (hipStream_t)stream, uniq, M, ncol, out, stride);
    return check_launch();
}

}  // namespace sky
}  // namespace jf

extern "C" {
int jf_sky_abi_version(void) { return 1; }
int jf_sky_vec2pix_f32(const float* v, int64_t stride, int32_t ncol, int64_t B, int32_t order, int64_t* pix_out, int32_t* status, void* s) {
    return jf::sky::vec2pix<float>(v, stride, ncol, B, order, pix_out, status, s);
}
int jf_sky_vec2pix_f64(const double* v, int64_t stride, int32_t ncol, int64_t B, int32_t order, int64_t* pix_out, int32_t* status, void* s) {
    return jf::sky::vec2pix<double>(v, stride, ncol, B, order, pix_out, status, s);
}
int jf_sky_cell_centres_f32(const int64_t* uniq, int64_t M, int32_t ncol, float* out, int64_t stride, void* s) {
    return jf::sky::cell_centres<float>(uniq, M, ncol, out, stride, s);
}
int jf_sky_cell_centres_f64(const int64_t* uniq, int64_t M, int32_t ncol, double* out, int64_t stride, void* s) {
    return jf::sky::cell_centres<double>(uniq, M, ncol, out, stride, s);
}
int jf_sky_cell_counts(const int64_t* sorted_pix, int64_t stride, int64_t G, int64_t S, const int64_t* uniq, const int64_t* row_of_cell,
                       int64_t n_cells, int64_t* counts, void* s) {
    using namespace jf::sky;
    if (!sorted_pix || !uniq || !row_of_cell || !counts || G < 0 || S < 0 || n_cells < 0 || stride < S) return JF_ERR_BADARG;
    if (n_cells > MAX_ELEMS || S > MAX_ELEMS) return JF_ERR_UNSUPPORTED;
    if (n_cells == 0) return JF_OK;
    jf::launch(cell_counts_kernel, dim3(blocks_of(n_cells)), dim3(THREADS), 0, (hipStream_t)s, sorted_pix, stride, G, S, uniq, row_of_cell,
               n_cells, counts);
    return jf::check_launch();
}
int jf_sky_locate(const int64_t* cell_start, const int64_t* offsets, int64_t G, const int64_t* pix, int64_t T, int64_t* cell_out, void* s) {
    using namespace jf::sky;
    if (!cell_start || !offsets || !pix || !cell_out || G < 0 || T < 0) return JF_ERR_BADARG;
    int64_t n = 0;
    if (__builtin_mul_overflow(G, T, &n) || n > MAX_ELEMS) return JF_ERR_UNSUPPORTED;
    if (n == 0) return JF_OK;
    jf::launch(locate_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)s, cell_start, offsets, G, pix, T, cell_out);
    return jf::check_launch();
}
}
