// stats3d.hip -- the 3-D flow statistics' running sums, for gfx950: one kernel
// family behind cfd_flow_stats3d_f32 (9 or 10 moments) and
// cfd_flow_scalar_stats3d_f32 (14 or 15), on (nz, ny, nx) float32 fields
// u, v, w, nu_t, T (x fastest) and float64 accumulators.
//
// The moments of a cell are u, v, w, uu, vv, ww, uv, uw, vw, then nu_t when it
// is given (NM = 10, 15), then with the passive scalar T, TT, uT, vT, wT
// (NM = 14, 15): each formed in double from the float32 values loaded (a
// product of two float32 values is exact in double) and added with a weight
// into the float64 sums.  No atomics and no workspace; the order of every sum
// depends on the shape alone: the same bits run to run.  NM only appends
// moments and one 4-byte load per cell; chunks, plane order, wave order and
// unroll are the same for all four counts, so the first 9 (10) planes of the
// 14 (15) moment call get the bits the 9 (10) moment call gives them.
//
// tests/stats3d_reference.py and tests/scalar_stats3d_reference.py state the
// arithmetic in NumPy.  All indexing is 64-bit.
#include "common.hpp"

namespace cfd {

constexpr bool stats_has_nut(int nm) { return nm == 10 || nm == 15; }
constexpr bool stats_has_T(int nm) { return nm > 10; }

// The kernels' inputs by value: T is a member only of the kernels that read
// it, so the 9 / 10 moment kernels keep their four-pointer argument list.
template <bool HAS_T>
struct StatsIn {
    const float *u, *v, *w, *nut;
};
template <>
struct StatsIn<true> {
    const float *u, *v, *w, *nut, *T;
};

// a: u, b: v, d: w, e: nu_t, f: T
template <int NM>
__device__ inline void stats_terms(float a, float b, float d, [[maybe_unused]] float e, [[maybe_unused]] float f,
                                   double (&t)[NM]) {
    static_assert(NM == 9 || NM == 10 || NM == 14 || NM == 15, "9, 10, 14 or 15 moments");
    constexpr int B = stats_has_T(NM) ? NM - 5 : NM;  // the moments without T's
    const double x = (double)a, y = (double)b, z = (double)d;
    t[0] = x;
    t[1] = y;
    t[2] = z;
    t[3] = x * x;
    t[4] = y * y;
    t[5] = z * z;
    t[6] = x * y;
    t[7] = x * z;
    t[8] = y * z;
    if constexpr (B == 10) t[9] = (double)e;
    if constexpr (stats_has_T(NM)) {
        const double s = (double)f;
        t[B] = s;
        t[B + 1] = s * s;
        t[B + 2] = x * s;
        t[B + 3] = y * s;
        t[B + 4] = z * s;
    }
}

// Span mode: acc[m, p] += weight * sum_k t_m(k, p) over the columns p of the
// (ny, nx) plane taken as one flat index (any nx: no row structure is used).
// A workgroup owns 64 adjacent columns; its kStatsWaves waves split z into
// contiguous chunks of ceil(nz / kStatsWaves) planes (the last ones may be
// short or empty).  Each wave marches its chunk in plane order, kStatsUnroll
// planes' loads issued together, into NM double sums per lane; the waves'
// partials meet in LDS and are added in wave order, multiplied by weight once
// and added to acc once.  So a column's sum is ((c_0 + c_1) + ...) + c_7 with
// c_q the in-order sum of chunk q.
//
// The combine, NM <= 10: one pass, part[8][NM][64], 36,864 / 40,960 B of LDS.
// NM > 10: the partials of all moments would take 8 * NM * 64 doubles (57,344 B
// at NM = 14), two workgroups per CU; they go through LDS in two halves of the
// moments instead (8 * ceil(NM / 2) * 64 doubles, 28,672 or 32,768 B), each
// added in wave order: the LDS traffic is reordered, no sum is.  Measured
// against the one-pass combine: 36.5 against 38.5 us (nm = 14), 42.7 against
// 46.1 us (nm = 15).  One pass is the same loop with a half of NM moments.
constexpr int kStatsWaves = 8;
// two planes: at four the span kernels hold 120 (nm = 9) and 158 (nm = 10) VGPRs and one or two
// workgroups fit a CU; at two they are faster at 600 x 180 x 120.  The same with T: at four
// 160 (nm = 14) and 236 (nm = 15) VGPRs and 47.9 and 56.6 us at 600 x 180 x 120 against 36.5
// and 42.7 us at two
constexpr int kStatsUnroll = 2;
constexpr unsigned kStatsMaxBlocks = 1u << 20;  // the kernels stride beyond
// moments per pass of the span combine and of full mode's accumulator updates
constexpr int stats_half(int nm) { return stats_has_T(nm) ? (nm + 1) / 2 : nm; }

template <int NM>
__global__ __launch_bounds__(kStatsWaves *kWave) void k_flow_stats3d_span(const StatsIn<stats_has_T(NM)> in,
                                                                          double *__restrict__ acc, int nz,
                                                                          size_t plane, size_t tiles, double weight) {
    constexpr int U = kStatsUnroll, H = stats_half(NM);
    constexpr bool NUT = stats_has_nut(NM), HAS_T = stats_has_T(NM);
    __shared__ double part[kStatsWaves][H][kWave];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int chunk = (nz + kStatsWaves - 1) / kStatsWaves;
    const int k0 = wv * chunk < nz ? wv * chunk : nz, k1 = k0 + chunk < nz ? k0 + chunk : nz;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t p = tile * kWave + lane;
        double s[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) s[m] = 0.0;
        if (p < plane) {
            size_t c = (size_t)k0 * plane + p;
            int k = k0;
            for (; k + U <= k1; k += U, c += U * plane) {
                float a[U], b[U], d[U], e[U], f[U];
#pragma unroll
                for (int q = 0; q < U; ++q) {
                    a[q] = in.u[c + q * plane];
                    b[q] = in.v[c + q * plane];
                    d[q] = in.w[c + q * plane];
                    e[q] = f[q] = 0.0f;
                    if constexpr (NUT) e[q] = in.nut[c + q * plane];
                    if constexpr (HAS_T) f[q] = in.T[c + q * plane];
                }
#pragma unroll
                for (int q = 0; q < U; ++q) {
                    double t[NM];
                    stats_terms<NM>(a[q], b[q], d[q], e[q], f[q], t);
#pragma unroll
                    for (int m = 0; m < NM; ++m) s[m] += t[m];
                }
            }
            for (; k < k1; ++k, c += plane) {
                float e = 0.0f, f = 0.0f;
                if constexpr (NUT) e = in.nut[c];
                if constexpr (HAS_T) f = in.T[c];
                double t[NM];
                stats_terms<NM>(in.u[c], in.v[c], in.w[c], e, f, t);
#pragma unroll
                for (int m = 0; m < NM; ++m) s[m] += t[m];
            }
        }
#pragma unroll
        for (int h = 0; h * H < NM; ++h) {
            const int m0 = h * H, mh = h == 0 ? H : NM - H;  // this pass: moments m0 .. m0 + mh - 1
#pragma unroll
            for (int m = 0; m < mh; ++m) part[wv][m][lane] = s[m0 + m];
            __syncthreads();
            for (int q = threadIdx.x; q < mh * kWave; q += kStatsWaves * kWave) {
                const int m = q / kWave, l = q % kWave;
                const size_t pp = tile * kWave + l;
                if (pp < plane) {
                    double r = part[0][m][l];
#pragma unroll
                    for (int x = 1; x < kStatsWaves; ++x) r += part[x][m][l];
                    const size_t o = (size_t)(m0 + m) * plane + pp;
                    acc[o] = acc[o] + weight * r;
                }
            }
            __syncthreads();  // part is rewritten by the next half or tile
        }
    }
}

// Full mode: acc[m, c] += weight * t_m(c), a read-modify-write of NM doubles
// per cell.  VEC (n even, fields 8-byte and acc 16-byte aligned): a thread
// takes two adjacent cells, the fields as float2 and each moment's
// accumulators as one 16-byte load and store; else one cell per thread.
template <int NM, bool VEC>
__global__ __launch_bounds__(256) void k_flow_stats3d_full(const StatsIn<stats_has_T(NM)> in,
                                                           double *__restrict__ acc, size_t n, double weight) {
    constexpr int C = VEC ? 2 : 1;
    constexpr bool NUT = stats_has_nut(NM), HAS_T = stats_has_T(NM);
    const size_t items = n / C;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < items; i += (size_t)gridDim.x * 256) {
        const size_t c = i * C;
        double t[C][NM];
        if constexpr (VEC) {
            const float2 a = *reinterpret_cast<const float2 *>(in.u + c), b = *reinterpret_cast<const float2 *>(in.v + c);
            const float2 d = *reinterpret_cast<const float2 *>(in.w + c);
            float2 e = {0.0f, 0.0f}, f = {0.0f, 0.0f};
            if constexpr (NUT) e = *reinterpret_cast<const float2 *>(in.nut + c);
            if constexpr (HAS_T) f = *reinterpret_cast<const float2 *>(in.T + c);
            stats_terms<NM>(a.x, b.x, d.x, e.x, f.x, t[0]);
            stats_terms<NM>(a.y, b.y, d.y, e.y, f.y, t[1]);
            // NM <= 10: all accumulators loaded first (H = NM).  NM > 10: in two halves of the
            // moments, 70 VGPRs against 128 (nm = 14) and 134 (nm = 15) with all of them loaded
            // first; the times did not tell the two apart
            constexpr int H = stats_half(NM);
#pragma unroll
            for (int m0 = 0; m0 < NM; m0 += H) {
                double2 o[H];
#pragma unroll
                for (int m = m0; m < m0 + H && m < NM; ++m)
                    o[m - m0] = *reinterpret_cast<const double2 *>(acc + (size_t)m * n + c);
#pragma unroll
                for (int m = m0; m < m0 + H && m < NM; ++m) {
                    o[m - m0].x = o[m - m0].x + weight * t[0][m];
                    o[m - m0].y = o[m - m0].y + weight * t[1][m];
                    *reinterpret_cast<double2 *>(acc + (size_t)m * n + c) = o[m - m0];
                }
            }
        } else {
            float e = 0.0f, f = 0.0f;
            if constexpr (NUT) e = in.nut[c];
            if constexpr (HAS_T) f = in.T[c];
            stats_terms<NM>(in.u[c], in.v[c], in.w[c], e, f, t[0]);
            double o[NM];
#pragma unroll
            for (int m = 0; m < NM; ++m) o[m] = acc[(size_t)m * n + c];
#pragma unroll
            for (int m = 0; m < NM; ++m) acc[(size_t)m * n + c] = o[m] + weight * t[0][m];
        }
    }
}

// one launch of the NM kernels: span (grid of tiles) or full (vec: two cells per thread)
template <int NM>
static void flow_stats3d_launch(bool span, bool vec, dim3 g, hipStream_t s, const float *u, const float *v,
                                const float *w, const float *nu_t, [[maybe_unused]] const float *T, double *acc,
                                int nz, size_t plane, size_t tiles, double weight) {
    StatsIn<stats_has_T(NM)> in;
    in.u = u;
    in.v = v;
    in.w = w;
    in.nut = nu_t;
    if constexpr (stats_has_T(NM)) in.T = T;
    const size_t n = plane * (size_t)nz;
    if (span)
        hipLaunchKernelGGL(k_flow_stats3d_span<NM>, g, dim3(kStatsWaves * kWave), 0, s, in, acc, nz, plane, tiles, weight);
    else if (vec)
        hipLaunchKernelGGL((k_flow_stats3d_full<NM, true>), g, dim3(256), 0, s, in, acc, n, weight);
    else
        hipLaunchKernelGGL((k_flow_stats3d_full<NM, false>), g, dim3(256), 0, s, in, acc, n, weight);
}

// cfd_flow_stats3d_f32 (T null) and, scalar, cfd_flow_scalar_stats3d_f32
static int flow_stats3d_run(const char *who, bool scalar, const float *u, const float *v, const float *w,
                            const float *nu_t, const float *T, double *acc, int nz, int ny, int nx, double weight,
                            int span_average, void *stream) {
    CFD_REQUIRE(u && v && w && acc && (T || !scalar), "%s: null pointer", who);
    CFD_REQUIRE(u != v && u != w && v != w, "%s: u, v, w must be three arrays", who);  // T may be one
    CFD_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, "%s: bad shape (%d, %d, %d): every dimension >= 1", who, nz, ny, nx);
    CFD_REQUIRE(weight - weight == 0.0, "%s: weight %g is not finite", who, weight);
    CFD_REQUIRE(span_average == 0 || span_average == 1, "%s: span_average %d is not 0 or 1", who, span_average);
    const size_t plane = (size_t)ny * nx, n = plane * (size_t)nz, tiles = (plane + kWave - 1) / kWave;
    auto al = [](const void *p_, uintptr_t m) { return ((uintptr_t)p_ & m) == 0; };  // null: aligned
    const bool vec = n % 2 == 0 && al(u, 7) && al(v, 7) && al(w, 7) && al(nu_t, 7) && al(T, 7) && al(acc, 15);
    const size_t blocks = span_average ? tiles : ((vec ? n / 2 : n) + 255) / 256;
    const dim3 g((unsigned)(blocks < kStatsMaxBlocks ? blocks : kStatsMaxBlocks));
    auto *launch = scalar ? (nu_t ? flow_stats3d_launch<15> : flow_stats3d_launch<14>)
                          : (nu_t ? flow_stats3d_launch<10> : flow_stats3d_launch<9>);
    launch(span_average != 0, vec, g, as_stream(stream), u, v, w, nu_t, T, acc, nz, plane, tiles, weight);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

}  // namespace cfd

using namespace cfd;

extern "C" {

int cfd_flow_stats3d_f32(const float *u, const float *v, const float *w, const float *nu_t, double *acc, int nz,
                         int ny, int nx, double weight, int span_average, void *stream) {
    return flow_stats3d_run("flow_stats3d_f32", false, u, v, w, nu_t, nullptr, acc, nz, ny, nx, weight, span_average,
                            stream);
}

int cfd_flow_scalar_stats3d_f32(const float *u, const float *v, const float *w, const float *nu_t, const float *T,
                                double *acc, int nz, int ny, int nx, double weight, int span_average, void *stream) {
    return flow_stats3d_run("flow_scalar_stats3d_f32", true, u, v, w, nu_t, T, acc, nz, ny, nx, weight,
                            span_average, stream);
}

}  // extern "C"
