// scalar3d.hip -- passive scalar (temperature) transport on the 3-D cylinder
// channel, for gfx950: the advance T_new = T + dt * (-conv + lap) and the
// heating / face stage, on (nz, ny, nx) float32 fields (x fastest).
//
// The arithmetic is the project's own (the reference has no scalar);
// tests/scalar3d_reference.py states it as NumPy float32 array code and the
// kernels reproduce it bit for bit.  The advance is the predictor's per-cell
// arithmetic (pred3_cell / pred3_tau, pred_planes.hpp, included unchanged)
// applied to T with the cell's diffusivity ae = alpha (+ nu_t * inv_prt) in
// place of nu; it runs as a plane march (scalar_planes.hpp) or one thread per
// cell, both with the same bits.  All indexing is 64-bit.
#include "common.hpp"
#include "internal.hpp"
#include "scalar_planes.hpp"

namespace cfd {

// One thread per cell (plain loads; the neighbours come from L1 / L2): any
// shape; the march's fallback and yardstick.  blockIdx.y = row, blockIdx.z =
// plane.  ZP: every plane is interior in z and the U / D neighbours wrap.
template <bool SUPG, bool NUT, bool ZP>
__global__ __launch_bounds__(256) void k_scalar_advance3d(const float *__restrict__ T, const float *__restrict__ u,
                                                          const float *__restrict__ v, const float *__restrict__ w,
                                                          float alpha, const float *__restrict__ nut, float inv_prt,
                                                          float *__restrict__ Tn, int nz, int ny, int nx, float dt,
                                                          PredK3 kk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    const int k = blockIdx.z;
    if (i >= nx) return;
    const size_t sy = (size_t)nx, sz = (size_t)ny * nx;
    const size_t c = ((size_t)k * ny + j) * nx + i;
    const float tc = T[c];
    float o = tc;  // the faces keep T
    if ((ZP || (k >= 1 && k < nz - 1)) && j >= 1 && j < ny - 1 && i >= 1 && i < nx - 1) {
        const size_t cu = ZP && k == nz - 1 ? c - (size_t)(nz - 1) * sz : c + sz;
        const size_t cd = ZP && k == 0 ? c + (size_t)(nz - 1) * sz : c - sz;
        const Nb7 f = {tc, T[c + 1], T[c - 1], T[c + sy], T[c - sy], T[cu], T[cd]};
        const float uc = u[c], vc = v[c], wc = w[c];
        float ae = alpha;
        if constexpr (NUT) ae = alpha + nut[c] * inv_prt;
        float t = 0.0f;
        if (SUPG) t = pred3_tau(uc, vc, wc, ae, dt, kk);
        o = pred3_cell<SUPG>(uc, vc, wc, f, t, ae, dt, kk);
    }
    Tn[c] = o;
}

// Heating of the scalar by the immersed boundary: relaxation towards t_cyl,
//   T = (float)((double)T + (m * fs) * (t_cyl - (double)T))
// on the cells of the mask's box [bi0, bi0 + bh) x [bj0, bj0 + bw) (already
// clipped to the non-face rows and columns) with m > 0, on planes kb ..
// kb + nk - 1 (the non-face planes).  One thread per visited cell, which reads
// and writes that cell alone.  heat (optional) += sum of (double)after -
// before: float64 per-thread sums, then the wave, the workgroup, one atomic
// per workgroup (skipped when the partial is 0).
struct Heat3 {
    float *T;
    const double *m;
    int ny, nx;
    double t_cyl, fs;
    int kb, nk, bi0, bj0, bh, bw;
    double *heat;
};

__global__ __launch_bounds__(256) void k_scalar_heat3d(Heat3 a) {
    __shared__ double part[4];
    double h = 0.0;
    const size_t sy = (size_t)a.nx, sz = (size_t)a.ny * a.nx;
    const size_t per = (size_t)a.bh * a.bw, total = per * (size_t)a.nk;
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t q = t % per;
        const int k = a.kb + (int)(t / per), i = a.bi0 + (int)(q / a.bw), j = a.bj0 + (int)(q % a.bw);
        const double mv = a.m[(size_t)i * sy + j];
        if (!(mv > 0.0)) continue;
        const size_t c = (size_t)k * sz + (size_t)i * sy + j;
        const double before = (double)a.T[c];
        const float after = (float)(before + (mv * a.fs) * (a.t_cyl - before));
        a.T[c] = after;
        h += (double)after - before;
    }
    if (!a.heat) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) h += __shfl_xor(h, off, kWave);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = ((part[0] + part[1]) + part[2]) + part[3];
        if (s != 0.0) atomicAdd(a.heat, s);  // a NaN is added too
    }
}

// The faces of the scalar, a pure gather (after the heating launch).  The
// ordered assignments -- spanwise faces plane 0 <- 1 and nz-1 <- nz-2,
// adiabatic walls row 0 <- 1 and ny-1 <- ny-2, outlet column nx-1 <- nx-2,
// inlet column 0 = t_in written last -- compose to: a face cell (k, i, j >= 1)
// takes the interior cell (clamp(k, 1, nz-2), clamp(i, 1, ny-2), min(j, nx-2)),
// a cell with j = 0 takes t_in.  One thread per face cell, in three disjoint
// ranges: planes 0 and nz-1 whole (none when ZP), rows 0 and ny-1 of the other
// planes, columns 0 and nx-1 of their rows 1 .. ny-2.  Written are face cells
// only, read are non-face cells only: no thread reads what another writes.
template <bool ZP>
__global__ __launch_bounds__(256) void k_scalar_faces3d(float *__restrict__ T, int nz, int ny, int nx, float t_in,
                                                        size_t n_plane, size_t n_rows, size_t n_cols) {
    const size_t sy = (size_t)nx, sz = (size_t)ny * nx;
    const size_t total = n_plane + n_rows + n_cols;
    constexpr int KB = ZP ? 0 : 1;  // first of the planes that are not faces
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        size_t r = t;
        int k, i, j;
        if (r < n_plane) {  // planes 0 and nz - 1
            k = r < sz ? 0 : nz - 1;
            const size_t q = r < sz ? r : r - sz;
            i = (int)(q / sy);
            j = (int)(q % sy);
        } else if ((r -= n_plane) < n_rows) {  // rows 0 and ny - 1
            k = KB + (int)(r / (2 * sy));
            const size_t q = r % (2 * sy);
            i = q < sy ? 0 : ny - 1;
            j = (int)(q % sy);
        } else {  // columns 0 and nx - 1 of rows 1 .. ny - 2
            r -= n_rows;
            const size_t per = 2 * (size_t)(ny - 2);
            k = KB + (int)(r / per);
            const size_t q = r % per;
            i = 1 + (int)(q >> 1);
            j = (q & 1) ? nx - 1 : 0;
        }
        float val = t_in;
        if (j != 0) {
            const int ks = ZP ? k : (k < 1 ? 1 : (k > nz - 2 ? nz - 2 : k));
            const int is = i < 1 ? 1 : (i > ny - 2 ? ny - 2 : i);
            const int js = j > nx - 2 ? nx - 2 : j;
            val = T[(size_t)ks * sz + (size_t)is * sy + js];
        }
        T[(size_t)k * sz + (size_t)i * sy + j] = val;
    }
}

static thread_local int g_last_scal3[2] = {-1, 0};

}  // namespace cfd

using namespace cfd;

// every dimension >= 3 (one interior cell), rows and planes within a launch grid
#define CFD_SCAL_SHAPE3D(who, nz, ny, nx)                                                                   \
    CFD_REQUIRE((nz) >= 3 && (ny) >= 3 && (nx) >= 3 && (ny) <= 65535 && (nz) <= 65535,                       \
                "%s: bad 3-D shape (nz, ny, nx) = (%d, %d, %d): every dimension 3 .. 65535 (nx: any >= 3)", who, \
                nz, ny, nx)
// periodic z: the two planes of a wrap have opposite red-black parity in the solver this serves
#define CFD_SCAL_ZPER(who, nz) \
    CFD_REQUIRE((nz) >= 4 && (nz) % 2 == 0, "%s: periodic z needs an even nz >= 4 (got nz = %d)", who, nz)

extern "C" {

static int scalar_advance3d_run(const char *who, bool zper, const float *T, const float *u, const float *v,
                                const float *w, float alpha, const float *nu_t, float inv_prt, float *T_new, int nz,
                                int ny, int nx, double dx, double dy, double dz, float dt, int use_supg,
                                void *stream) {
    CFD_REQUIRE(T, "%s: null pointer: T", who);
    CFD_REQUIRE(u, "%s: null pointer: u", who);
    CFD_REQUIRE(v, "%s: null pointer: v", who);
    CFD_REQUIRE(w, "%s: null pointer: w", who);
    CFD_REQUIRE(T_new, "%s: null pointer: T_new", who);
    CFD_SCAL_SHAPE3D(who, nz, ny, nx);
    if (zper) CFD_SCAL_ZPER(who, nz);
    CFD_REQUIRE(T_new != T, "%s: T_new must not alias T", who);
    CFD_REQUIRE(T_new != u, "%s: T_new must not alias u", who);
    CFD_REQUIRE(T_new != v, "%s: T_new must not alias v", who);
    CFD_REQUIRE(T_new != w, "%s: T_new must not alias w", who);
    CFD_REQUIRE(T_new != nu_t, "%s: T_new must not alias nu_t", who);
    const PredK3 k = make_pred_k3(dx, dy, dz);
    hipStream_t s = as_stream(stream);
    // cells per lane of the plane march: the preferred count (tuning; auto: 2,
    // the fastest measured shape with 2 rows per wave at 600 x 180 x 120, where
    // 4 cells per lane holds 117 .. 158 VGPRs and is the slowest: DESIGN.md
    // 4.6), halved until nx and every array's alignment allow it (1 always does)
    int vec = tuning().scal3_vec;
    if (!vec) vec = 2;
    auto fits = [&](int c) {
        const uintptr_t m = (uintptr_t)(4 * c - 1);
        auto al = [&](const void *p_) { return !p_ || ((uintptr_t)p_ & m) == 0; };
        return nx % c == 0 && al(T) && al(u) && al(v) && al(w) && al(nu_t) && al(T_new);
    };
    while (vec > 1 && !fits(vec)) vec /= 2;
    // the predictor's march conditions: a plane's byte offsets fit its buffer
    // resource and (auto) nx and the alignment leave more than one cell per
    // lane; a forced march (variant 2) also runs at one
    const bool plane_ok = (size_t)ny * nx * sizeof(float) < ((size_t)1 << 31);
    const int variant = tuning().scal3_variant;
    const bool march = plane_ok && variant != 1 && (variant == 2 || vec > 1);
    if (march) {
        Scalar3Args a;
        a.T = T;
        a.u = u;
        a.v = v;
        a.w = w;
        a.nut = nu_t;
        a.Tn = T_new;
        a.alpha = alpha;
        a.inv_prt = inv_prt;
        a.dt = dt;
        a.nz = nz;
        a.ny = ny;
        a.nx = nx;
        a.k = k;
        const int rows = tuning().scal3_rows ? tuning().scal3_rows : 2;
        CFD_CHECK_HIP(scalar_planes_launch(a, use_supg != 0, zper, vec, rows, tuning().scal3_zchunk, s));
        g_last_scal3[0] = 1;
        g_last_scal3[1] = vec;
    } else {
        const dim3 g(ceil_div(nx, 256), ny, nz);
#define CFD_SCAL3_CELL(SUPG, NUT, ZP)                                                                            \
    hipLaunchKernelGGL((k_scalar_advance3d<SUPG, NUT, ZP>), g, dim3(256), 0, s, T, u, v, w, alpha, nu_t, inv_prt, \
                       T_new, nz, ny, nx, dt, k)
#define CFD_SCAL3_CELL_Z(SUPG, NUT)            \
    do {                                       \
        if (zper) CFD_SCAL3_CELL(SUPG, NUT, true); \
        else CFD_SCAL3_CELL(SUPG, NUT, false); \
    } while (0)
        if (use_supg) {
            if (nu_t) CFD_SCAL3_CELL_Z(true, true);
            else CFD_SCAL3_CELL_Z(true, false);
        } else {
            if (nu_t) CFD_SCAL3_CELL_Z(false, true);
            else CFD_SCAL3_CELL_Z(false, false);
        }
#undef CFD_SCAL3_CELL_Z
#undef CFD_SCAL3_CELL
        g_last_scal3[0] = 0;
        g_last_scal3[1] = 1;
    }
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_scalar_advance3d_f32(const float *T, const float *u, const float *v, const float *w, float alpha,
                             const float *nu_t, float inv_prt, float *T_new, int nz, int ny, int nx, double dx,
                             double dy, double dz, float dt, int use_supg, void *stream) {
    return scalar_advance3d_run("scalar_advance3d", false, T, u, v, w, alpha, nu_t, inv_prt, T_new, nz, ny, nx, dx,
                                dy, dz, dt, use_supg, stream);
}

int cfd_scalar_advance3d_zper_f32(const float *T, const float *u, const float *v, const float *w, float alpha,
                                  const float *nu_t, float inv_prt, float *T_new, int nz, int ny, int nx, double dx,
                                  double dy, double dz, float dt, int use_supg, void *stream) {
    return scalar_advance3d_run("scalar_advance3d_zper", true, T, u, v, w, alpha, nu_t, inv_prt, T_new, nz, ny, nx,
                                dx, dy, dz, dt, use_supg, stream);
}

int cfd_set_scalar3d_config(int variant, int rows, int cells_per_lane, int zchunk) {
    CFD_REQUIRE(variant >= 0 && variant <= 2, "scalar3d config: variant 0 (auto), 1 (per cell) or 2 (plane march)");
    CFD_REQUIRE(rows == 0 || rows == 1 || rows == 2, "scalar3d config: rows per wave 0 (auto), 1 or 2");
    CFD_REQUIRE(cells_per_lane == 0 || cells_per_lane == 1 || cells_per_lane == 2 || cells_per_lane == 4,
                "scalar3d config: cells per lane 0 (auto), 1, 2 or 4");
    CFD_REQUIRE(zchunk >= 0 && zchunk <= 65535, "scalar3d config: planes per chunk 0 (auto) .. 65535");
    tuning().scal3_variant = variant;
    tuning().scal3_rows = rows;
    tuning().scal3_vec = cells_per_lane;
    tuning().scal3_zchunk = zchunk;
    return CFD_OK;
}

int cfd_get_last_scalar3d_path(int *cells_per_lane) {
    if (cells_per_lane) *cells_per_lane = g_last_scal3[1];
    return g_last_scal3[0];
}

static int scalar_bc_heat3d_run(const char *who, bool zper, float *T, const double *ibm_mask2d, int nz, int ny,
                                int nx, double t_in, double t_cyl, double force_strength, int i0, int i1, int j0,
                                int j1, double *heat_out, void *stream) {
    CFD_REQUIRE(T, "%s: null pointer: T", who);
    CFD_SCAL_SHAPE3D(who, nz, ny, nx);
    if (zper) CFD_SCAL_ZPER(who, nz);
    CFD_REQUIRE(i0 >= 0 && i0 <= i1 && i1 <= ny && j0 >= 0 && j0 <= j1 && j1 <= nx,
                "%s: box [%d, %d) x [%d, %d) outside the (%d, %d) plane", who, i0, i1, j0, j1, ny, nx);
    CFD_REQUIRE(!ibm_mask2d || (i0 < i1 && j0 < j1), "%s: empty box [%d, %d) x [%d, %d) with a mask", who, i0, i1,
                j0, j1);
    hipStream_t s = as_stream(stream);
    const size_t cap = (size_t)1 << 20;  // the kernels stride beyond
    // the planes that are not faces, and the box clipped to the non-face rows and columns
    const int kb = zper ? 0 : 1, nk = zper ? nz : nz - 2;
    const int bi0 = i0 > 1 ? i0 : 1, bi1 = i1 < ny - 1 ? i1 : ny - 1;
    const int bj0 = j0 > 1 ? j0 : 1, bj1 = j1 < nx - 1 ? j1 : nx - 1;
    const int bh = bi1 > bi0 ? bi1 - bi0 : 0, bw = bj1 > bj0 ? bj1 - bj0 : 0;
    if (ibm_mask2d && bh > 0 && bw > 0) {
        Heat3 a;
        a.T = T;
        a.m = ibm_mask2d;
        a.ny = ny;
        a.nx = nx;
        a.t_cyl = t_cyl;
        a.fs = force_strength;
        a.kb = kb;
        a.nk = nk;
        a.bi0 = bi0;
        a.bj0 = bj0;
        a.bh = bh;
        a.bw = bw;
        a.heat = heat_out;
        size_t blocks = ((size_t)bh * bw * (size_t)nk + 255) / 256;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(k_scalar_heat3d, dim3((unsigned)blocks), dim3(256), 0, s, a);
    }
    const size_t n_plane = zper ? 0 : 2 * (size_t)ny * nx;
    const size_t n_rows = (size_t)nk * 2 * (size_t)nx, n_cols = (size_t)nk * 2 * (size_t)(ny - 2);
    size_t blocks = (n_plane + n_rows + n_cols + 255) / 256;
    if (blocks > cap) blocks = cap;
    if (zper)
        hipLaunchKernelGGL(k_scalar_faces3d<true>, dim3((unsigned)blocks), dim3(256), 0, s, T, nz, ny, nx, (float)t_in,
                           n_plane, n_rows, n_cols);
    else
        hipLaunchKernelGGL(k_scalar_faces3d<false>, dim3((unsigned)blocks), dim3(256), 0, s, T, nz, ny, nx, (float)t_in,
                           n_plane, n_rows, n_cols);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_scalar_bc_heat3d_f32(float *T, const double *ibm_mask2d, int nz, int ny, int nx, double t_in, double t_cyl,
                             double force_strength, int i0, int i1, int j0, int j1, double *heat_out, void *stream) {
    return scalar_bc_heat3d_run("scalar_bc_heat3d", false, T, ibm_mask2d, nz, ny, nx, t_in, t_cyl, force_strength, i0,
                                i1, j0, j1, heat_out, stream);
}

int cfd_scalar_bc_heat3d_zper_f32(float *T, const double *ibm_mask2d, int nz, int ny, int nx, double t_in,
                                  double t_cyl, double force_strength, int i0, int i1, int j0, int j1,
                                  double *heat_out, void *stream) {
    return scalar_bc_heat3d_run("scalar_bc_heat3d_zper", true, T, ibm_mask2d, nz, ny, nx, t_in, t_cyl, force_strength,
                                i0, i1, j0, j1, heat_out, stream);
}

}  // extern "C"
