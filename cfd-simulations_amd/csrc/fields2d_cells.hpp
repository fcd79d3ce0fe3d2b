// fields2d_cells.hpp -- the one-thread-per-cell kernels of the v5 cylinder
// solver's time_step() (v5.py:375-441) and their host launchers, once, as
// templates on the field type T: float (memory_efficient=True, fields2d.hip)
// or double (fields2d_f64.hip).  Each extern "C" entry point of the two files
// is one call of a launcher here, with its own name as `who` for the errors.
//
// Arithmetic follows the reference as it executes in NumPy-scalar form
// (NEP 50): a Python-float constant is rounded to T where it meets T data --
// the launchers form every constant in double and cast it to T once, which for
// double changes nothing -- and the operations run in T in the source order,
// nothing fused (-ffp-contract=off).  The literals in the kernels (0, 0.5, 1,
// 2) are exact in both types.  The one operation that differs between the
// types is the SUPG |V| (vel_mag below).
//
// These kernels are one-pass per cell and HBM-bound; the fused predictor
// reads u, v once (5-point neighbourhoods from L1/L2) and writes u*, v*, tau.
#pragma once
#include <limits>

#include "common.hpp"
#include "internal.hpp"
#include "libm_pow.hpp"
#include "libm_powf.hpp"
#include "pred_rows.hpp"

namespace cfd {

// |V| = (u**2 + v**2) ** 0.5 on NumPy scalars, v5.py:155: libm's power three
// times.  float32: glibc's powf (powf_sq / powf_sqrt: powf at y = 2 / 0.5 bit
// for bit, with a cheap exact path away from rounding midpoints --
// libm_powf.hpp).  float64: glibc's pow, which is not correctly rounded (on
// ~1e-3 of random inputs pow(x, 2) != x*x and pow(x, 0.5) != sqrt(x)), as its
// device restatement (libm_pow.hpp).  So both steps are bit-exact against the
// reference's own.
__device__ inline float vel_mag(float u, float v) {
    const libm::PowfTables &T = libm::kPowfTables;
    return libm::powf_sqrt(libm::powf_sq(u, T) + libm::powf_sq(v, T), T);
}
__device__ inline double vel_mag(double u, double v) {
    return libm::pow(libm::pow(u, 2.0) + libm::pow(v, 2.0), 0.5);
}
__device__ inline float abs_ieee(float x) { return __builtin_fabsf(x); }
__device__ inline double abs_ieee(double x) { return __builtin_fabs(x); }

// compute_supg_stabilization_fast body, v5.py:155-161; tau = dt / 2 is exact
// (dt is a float32, or a double that meets float64 fields exactly)
template <typename T>
__device__ inline T supg_tau(T u, T v, T nu, T dt, const PredK<T> &k) {
    const T vm = vel_mag(u, v);
    if (vm > k.eps) {
        const T pe = (vm * k.h) / (nu + k.eps);
        const T half = pe / T(2);
        const T lim = half < T(1) ? half : T(1);  // Python min(1.0, Pe/2.0)
        return (k.h / (T(2) * vm)) * lim;
    }
    return dt / T(2);
}
__device__ inline bool interior(int i, int j, int ny, int nx) {
    return i >= 1 && i < ny - 1 && j >= 1 && j < nx - 1;
}

#define CFD_2D_INDEX                                     \
    const int j = blockIdx.x * blockDim.x + threadIdx.x; \
    const int i = blockIdx.y;                            \
    if (j >= nx) return;                                 \
    const size_t c = (size_t)i * nx + j;

template <typename T>
__global__ void k_supg_tau(const T *__restrict__ u, const T *__restrict__ v, const T *__restrict__ nu_eff, T nu_s,
                           T *__restrict__ tau, int ny, int nx, T dt, PredK<T> k) {
    CFD_2D_INDEX
    T t = T(0);  // np.zeros_like boundary ring
    if (interior(i, j, ny, nx)) t = supg_tau(u[c], v[c], nu_eff ? nu_eff[c] : nu_s, dt, k);
    tau[c] = t;
}

template <typename T>
__global__ void k_conv_supg(const T *__restrict__ u, const T *__restrict__ v, const T *__restrict__ f,
                            const T *__restrict__ tau, T *__restrict__ conv, int ny, int nx, PredK<T> k) {
    CFD_2D_INDEX
    T r = T(0);
    if (interior(i, j, ny, nx))
        r = conv_supg(u[c], v[c], f[c], f[c + 1], f[c - 1], f[c + nx], f[c - nx], tau[c], k);
    conv[c] = r;
}

template <typename T>
__global__ void k_conv_upwind(const T *__restrict__ u, const T *__restrict__ v, const T *__restrict__ f,
                              T *__restrict__ conv, int ny, int nx, PredK<T> k) {
    CFD_2D_INDEX
    T r = T(0);
    if (interior(i, j, ny, nx))
        r = conv_upwind(u[c], v[c], f[c], f[c + 1], f[c - 1], f[c + nx], f[c - nx], k);
    conv[c] = r;
}

template <typename T>
__global__ void k_laplacian(const T *__restrict__ f, const T *__restrict__ nu_eff, T nu_s, T *__restrict__ lap,
                            int ny, int nx, PredK<T> k) {
    CFD_2D_INDEX
    T r = T(0);
    if (interior(i, j, ny, nx))
        r = laplacian(nu_eff ? nu_eff[c] : nu_s, f[c], f[c + 1], f[c - 1], f[c + nx], f[c - nx], k);
    lap[c] = r;
}

// compute_smagorinsky_viscosity_fast, v5.py:96-110 (smag_nut, pred_rows.hpp)
template <typename T>
__global__ void k_smagorinsky(const T *__restrict__ u, const T *__restrict__ v, T *__restrict__ nut, int ny, int nx,
                              T cles, PredK<T> k) {
    CFD_2D_INDEX
    T r = T(0);
    if (interior(i, j, ny, nx)) r = smag_nut(u[c], v[c], u[c + 1], v[c + 1], u[c + nx], v[c + nx], cles, k);
    nut[c] = r;
}

// Fused predictor, v5.py:388-403: u* = u + dt*(-conv_u + lap_u), likewise v.
// LES: nu_eff holds nu_t and nu_eff = (nu_s + nu_t) + art per cell (v5.py:388).
template <typename T, bool SUPG, bool LES>
__global__ __launch_bounds__(256) void k_predictor(const T *__restrict__ u, const T *__restrict__ v,
                                                   const T *__restrict__ nu_eff, T nu_s, T *__restrict__ us,
                                                   T *__restrict__ vs, T *__restrict__ tau_out, int ny, int nx,
                                                   T dt, PredK<T> k, T art) {
    CFD_2D_INDEX
    const T uc = u[c], vc = v[c];
    T cu = T(0), cv = T(0), lu = T(0), lv = T(0), t = T(0);
    if (interior(i, j, ny, nx)) {
        const T nu = LES ? (nu_s + nu_eff[c]) + art : (nu_eff ? nu_eff[c] : nu_s);
        const T uE = u[c + 1], uW = u[c - 1], uN = u[c + nx], uS = u[c - nx];
        const T vE = v[c + 1], vW = v[c - 1], vN = v[c + nx], vS = v[c - nx];
        if (SUPG) {
            t = supg_tau(uc, vc, nu, dt, k);
            cu = conv_supg(uc, vc, uc, uE, uW, uN, uS, t, k);
            cv = conv_supg(uc, vc, vc, vE, vW, vN, vS, t, k);
        } else {
            cu = conv_upwind(uc, vc, uc, uE, uW, uN, uS, k);
            cv = conv_upwind(uc, vc, vc, vE, vW, vN, vS, k);
        }
        lu = laplacian(nu, uc, uE, uW, uN, uS, k);
        lv = laplacian(nu, vc, vE, vW, vN, vS, k);
    }
    us[c] = uc + dt * (-cu + lu);
    vs[c] = vc + dt * (-cv + lv);
    if (tau_out) tau_out[c] = t;  // 0 without SUPG (v5.py:292: never assigned without SUPG)
}

// compute_divergence_fast, v5.py:178-187 (+ max|div| diagnostic, v5.py:410)
template <typename T>
__global__ __launch_bounds__(256) void k_divergence(const T *__restrict__ u, const T *__restrict__ v,
                                                    T *__restrict__ div, int ny, int nx, T cx, T cy, T *absmax) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    T m = T(0);
    if (j < nx) {
        const size_t c = (size_t)i * nx + j;
        T d = T(0);
        if (interior(i, j, ny, nx)) d = (u[c + 1] - u[c - 1]) * cx + (v[c + nx] - v[c - nx]) * cy;
        div[c] = d;
        const T a = abs_ieee(d);
        if (a > m) m = a;
    }
    if (absmax) wave_reduce_max_store(m, absmax);
}

// compute_gradient_fast, v5.py:189-200
template <typename T>
__global__ void k_gradient(const T *__restrict__ phi, T *__restrict__ gx, T *__restrict__ gy, int ny, int nx, T cx,
                           T cy) {
    CFD_2D_INDEX
    T a = T(0), b = T(0);
    if (interior(i, j, ny, nx)) {
        a = (phi[c + 1] - phi[c - 1]) * cx;
        b = (phi[c + nx] - phi[c - nx]) * cy;
    }
    gx[c] = a;
    gy[c] = b;
}

// v5.py:413-417: gradient of phi, then u = u* - dt*dpdx, v = v* - dt*dpdy;
// gradmax <- max sqrt(dpdx^2 + dpdy^2) (v5.py:414-415 diagnostic).
template <typename T>
__global__ __launch_bounds__(256) void k_project(const T *__restrict__ phi, const T *__restrict__ us,
                                                 const T *__restrict__ vs, T *__restrict__ u, T *__restrict__ v,
                                                 int ny, int nx, T cx, T cy, T dt, T *gradmax) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    T m = T(0);
    if (j < nx) {
        const size_t c = (size_t)i * nx + j;
        T a = T(0), b = T(0);
        if (interior(i, j, ny, nx)) {
            a = (phi[c + 1] - phi[c - 1]) * cx;
            b = (phi[c + nx] - phi[c - nx]) * cy;
        }
        u[c] = us[c] - dt * a;
        v[c] = vs[c] - dt * b;
        if (gradmax) {
            const T g = sqrt_ieee(a * a + b * b);
            if (g > m) m = g;
        }
    }
    if (gradmax) wave_reduce_max_store(m, gradmax);
}

// clean_divergence_fast's phi sweep (v5.py:250-253) in the serial
// lexicographic order (under prange the reference races; the serial loop is
// the semantics this library defines): a single workgroup walks the
// anti-diagonals; every cell of a diagonal depends only on earlier diagonals
// (W, S: new) and later ones (E, N: old), so updating one diagonal at a time
// reproduces the serial loop exactly.  Thread t owns row b0 + t of a band of
// blockDim rows and updates column st - t + 1 at step st; W is its own last
// output (a register), S thread t-1's output one step earlier (LDS,
// double-buffered by step parity, one barrier per step), E / N / div are old
// values read from memory.  The float64 step's sweep; float32 grids take it
// only past the skewed sweep's 2^31-byte offsets (fields2d.hip).
template <typename T>
__global__ __launch_bounds__(1024) void k_lex_gs_sweep(T *__restrict__ phi, const T *__restrict__ div, int ny,
                                                       int nx, T cx, T cy, T cd) {
    __shared__ T outb[2][1024];
    const int t = threadIdx.x, nt = blockDim.x;
    const int imax = ny - 2, jmax = nx - 2;
    for (int b0 = 1; b0 <= imax; b0 += nt) {
        __threadfence();  // the previous band's rows are final and visible
        __syncthreads();
        const int nrows = min(nt, imax - b0 + 1);
        const int i = b0 + t;
        const bool rowok = t < nrows;
        const size_t rowc = (size_t)(rowok ? i : 0) * nx;
        T w = rowok ? phi[rowc] : T(0);  // phi(i, 0): W of column 1
        const int nsteps = nrows - 1 + jmax;
        for (int st = 0; st < nsteps; ++st) {
            const int j = st - t + 1;
            if (rowok && j >= 1 && j <= jmax) {
                const T E = phi[rowc + j + 1];
                const T N = phi[rowc + j + nx];  // old (row i+1 is behind)
                const T S = t == 0 ? phi[rowc + j - nx] : outb[(st + 1) & 1][t - 1];
                const T a = cx * (E + w);
                const T b = cy * (N + S);
                const T val = ((a + b) - div[rowc + j]) * cd;
                phi[rowc + j] = val;
                w = val;
                outb[st & 1][t] = val;
            }
            __syncthreads();
        }
    }
}

// u[1:-1,1:-1] -= grad_x[1:-1,1:-1] (no dt: v5.py:255-256)
template <typename T>
__global__ void k_sub_gradient(const T *__restrict__ phi, T *__restrict__ u, T *__restrict__ v, int ny, int nx,
                               T cx, T cy) {
    CFD_2D_INDEX
    if (!interior(i, j, ny, nx)) return;
    const T a = (phi[c + 1] - phi[c - 1]) * cx;
    const T b = (phi[c + nx] - phi[c - nx]) * cy;
    u[c] = u[c] - a;
    v[c] = v[c] - b;
}

// apply_boundary_conditions, v5.py:349-360.  Net effect of the eight
// assignments in order: rows 0 and ny-1 end at 0; other rows get the inlet
// u = T(V_inf*(1 + pert_scale*sin(2*pi*y/y_max + 0.02*step))), v = 0 at
// x = 0 and a zero-gradient outlet copy from x = nx-2.
template <typename T>
__global__ void k_bc(T *__restrict__ u, T *__restrict__ v, const double *__restrict__ y, int ny, int nx,
                     double y_max, double v_inf, int step) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nx) {  // top / bottom rows
        u[t] = T(0);
        v[t] = T(0);
        u[(size_t)(ny - 1) * nx + t] = T(0);
        v[(size_t)(ny - 1) * nx + t] = T(0);
    }
    const int i = t;
    if (i >= 1 && i < ny - 1) {
        const double s = (double)step;
        double scale = s / 1000.0;
        scale = (1.0 < scale ? 1.0 : scale) * 0.01;
        const double two_pi = 2.0 * 3.141592653589793;
        const double pert = scale * sin(two_pi * y[i] / y_max + 0.02 * s);
        const size_t r = (size_t)i * nx;
        u[r] = (T)(v_inf * (1.0 + pert));
        v[r] = T(0);
        u[r + nx - 1] = u[r + nx - 2];
        v[r + nx - 1] = v[r + nx - 2];
    }
}

// Lid-driven cavity walls (BASELINE config 1; the reference has no
// incompressible cavity, so the walls follow the assignment pattern of
// v5.py:349-360): no-slip u = v = 0 on the left, right and bottom walls, the
// lid u = u_lid, v = 0 on the top row y = y_max (row ny-1), the lid written
// last so it owns the two top corners.
template <typename T>
__global__ void k_lid_bc(T *__restrict__ u, T *__restrict__ v, int ny, int nx, T u_lid) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ny - 1) {  // side walls, rows 0 .. ny-2
        const size_t r = (size_t)t * nx;
        u[r] = T(0);
        v[r] = T(0);
        u[r + nx - 1] = T(0);
        v[r + nx - 1] = T(0);
    }
    if (t < nx) {
        u[t] = T(0);  // bottom wall
        v[t] = T(0);
        u[(size_t)(ny - 1) * nx + t] = u_lid;  // lid
        v[(size_t)(ny - 1) * nx + t] = T(0);
    }
}

// apply_ibm_fast, v5.py:228-237 (ibm_cell: float64 mask => float64 arithmetic)
template <typename T>
__global__ void k_ibm(T *__restrict__ u, T *__restrict__ v, const double *__restrict__ m, int n, double fs) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
        const double mv = m[c];
        if (mv > 0.0) {
            u[c] = ibm_cell(u[c], mv, fs);
            v[c] = ibm_cell(v[c], mv, fs);
        }
    }
}

template <typename T>
__global__ void k_clip(T *__restrict__ a, size_t n, T lo, T hi) {
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
        const T x = a[c];
        a[c] = x < lo ? lo : (x > hi ? hi : x);  // NaN passes through like np.clip
    }
}

// ------------------------------------------------------------ reductions
template <typename T>
__global__ void k_absmax(const T *__restrict__ a, const T *__restrict__ b, size_t n, T *out) {
    T m = T(0);
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
        T x = abs_ieee(a[c]);
        if (x > m) m = x;
        if (b) {
            x = abs_ieee(b[c]);
            if (x > m) m = x;
        }
    }
    wave_reduce_max_store(m, out);
}

// sum of 0.5*(u^2 + v^2) (v5.py:362-363, :431-432), scaled by 1/n after; each
// cell's energy in T like NumPy, the sum in float64.
template <typename T>
__global__ void k_energy_sum(const T *__restrict__ u, const T *__restrict__ v, size_t n, double *out) {
    double s = 0.0;
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
        const T e = T(0.5) * (u[c] * u[c] + v[c] * v[c]);
        s += (double)e;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, kWave);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, s);
}

static __global__ void k_scale_double(double *p, double f) { *p = *p * f; }

// compute_vorticity (v5.py:365-373): interior central differences, boundary
// ring 0, masked cells NaN, into w (when given); nanmax|w| (v5.py:427-428:
// masked cells skipped) into absmax (when given).
template <typename T>
__global__ void k_vorticity(const T *__restrict__ u, const T *__restrict__ v, const uint8_t *__restrict__ mask,
                            T *__restrict__ w, int ny, int nx, T dx2, T dy2, T *absmax) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    T m = T(0);
    if (j < nx) {
        const size_t c = (size_t)i * nx + j;
        T r = T(0);
        if (interior(i, j, ny, nx)) r = (v[c + 1] - v[c - 1]) / dx2 - (u[c + nx] - u[c - nx]) / dy2;
        const bool masked = mask && mask[c];
        if (w) w[c] = masked ? std::numeric_limits<T>::quiet_NaN() : r;
        if (!masked && abs_ieee(r) > m) m = abs_ieee(r);
    }
    if (absmax) wave_reduce_max_store(m, absmax);
}

template <typename T>
__global__ void k_nonfinite(const T *__restrict__ a, const T *__restrict__ b, size_t n, int *out) {
    int cnt = 0;
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
        cnt += !isfinite(a[c]);
        if (b) cnt += !isfinite(b[c]);
    }
    if (cnt) atomicAdd(out, cnt);
}

// ------------------------------------------------------------ launchers
inline dim3 grid2d(int ny, int nx) { return dim3(ceil_div(nx, 256), ny); }
inline int grid1d(size_t n) {
    long b = (long)((n + 255) / 256);
    if (b > 2048) b = 2048;
    if (b < 1) b = 1;
    return (int)b;
}

#define CFD_SHAPE2D(ny, nx) CFD_REQUIRE((ny) >= 1 && (nx) >= 1, "bad 2-D shape (%d, %d)", ny, nx)

template <typename T>
int supg_tau2d(const char *who, const T *u, const T *v, const T *nu_eff, T nu_s, T *tau, int ny, int nx, double dx,
               double dy, T dt, void *stream) {
    CFD_REQUIRE(u && v && tau, "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_supg_tau<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), u, v, nu_eff, nu_s, tau, ny,
                       nx, dt, make_pred_k<T>(dx, dy));
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int convection_supg2d(const char *who, const T *u, const T *v, const T *phi, const T *tau, T *conv, int ny, int nx,
                      double dx, double dy, void *stream) {
    CFD_REQUIRE(u && v && phi && tau && conv, "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_conv_supg<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), u, v, phi, tau, conv, ny, nx,
                       make_pred_k<T>(dx, dy));
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int convection_upwind2d(const char *who, const T *u, const T *v, const T *phi, T *conv, int ny, int nx, double dx,
                        double dy, void *stream) {
    CFD_REQUIRE(u && v && phi && conv, "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_conv_upwind<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), u, v, phi, conv, ny, nx,
                       make_pred_k<T>(dx, dy));
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int laplacian2d(const char *who, const T *phi, const T *nu_eff, T nu_s, T *lap, int ny, int nx, double dx, double dy,
                void *stream) {
    CFD_REQUIRE(phi && lap, "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_laplacian<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), phi, nu_eff, nu_s, lap, ny,
                       nx, make_pred_k<T>(dx, dy));
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int smagorinsky2d(const char *who, const T *u, const T *v, T *nu_t, int ny, int nx, double dx, double dy, double cs,
                  void *stream) {
    CFD_REQUIRE(u && v && nu_t, "%s: null pointer", who);
    CFD_REQUIRE(nu_t != u && nu_t != v, "%s: nu_t must not alias an input", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_smagorinsky<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), u, v, nu_t, ny, nx,
                       (T)smag_const(cs, dx, dy), make_pred_k<T>(dx, dy));
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

// cfd_predictor2d_* (les == false) and cfd_predictor2d_les_* (nu_eff null,
// nu_s the molecular nu; nu_t may be null on the row march)
template <typename T>
int predictor2d(const char *who, const T *u, const T *v, const T *nu_eff, T nu_s, T *u_star, T *v_star, T *tau,
                int ny, int nx, double dx, double dy, T dt, int use_supg, void *stream, bool les, T art, double cs,
                T *nu_t) {
    CFD_REQUIRE(u && v && u_star && v_star, "%s: null pointer", who);
    CFD_REQUIRE(u_star != u && v_star != v && u_star != v && v_star != u, "%s: outputs must not alias inputs", who);
    CFD_REQUIRE(!nu_t || (nu_t != u && nu_t != v && nu_t != u_star && nu_t != v_star && nu_t != tau),
                "%s: nu_t must not alias another array", who);
    CFD_SHAPE2D(ny, nx);
    const PredK<T> k = make_pred_k<T>(dx, dy);
    const T cles = les ? (T)smag_const(cs, dx, dy) : T(0);
    hipStream_t s = as_stream(stream);
    // cells per lane of the row march (pred_rows.hpp): the preferred count
    // (tuning; default 2; 16 B per lane at most: float 4, double 2), halved
    // until nx and every array's alignment allow it
    int vec = tuning().pred_vec ? tuning().pred_vec : 2;
    if (vec > (int)(16 / sizeof(T))) vec = (int)(16 / sizeof(T));
    auto fits = [&](int w) {
        const uintptr_t m = (uintptr_t)(sizeof(T) * w - 1);
        auto al = [&](const void *p_) { return !p_ || ((uintptr_t)p_ & m) == 0; };
        return nx % w == 0 && al(u) && al(v) && al(u_star) && al(v_star) && al(tau) && al(nu_eff) && al(nu_t);
    };
    while (vec > 1 && !fits(vec)) vec /= 2;
    const bool rows_ok = (size_t)ny * nx * sizeof(T) < ((size_t)1 << 31) && fits(vec);
    const bool rows = tuning().pred_variant != 1 && rows_ok;
    CFD_REQUIRE(!les || rows || nu_t, "%s: the one-thread-per-cell path needs nu_t (it stores it, then reads it)",
                who);
    const int tau_mode = use_supg ? tuning().pred_tau : kTauExact;
    const int tk = timing_begin(s, kTimingPredictor);
    if (rows) {
        PredRowArgs<T> a;
        a.u = u;
        a.v = v;
        a.nu = nu_eff;
        a.us = u_star;
        a.vs = v_star;
        a.tau = tau;  // zeros without SUPG
        a.nu_s = nu_s;
        a.dt = dt;
        a.ny = ny;
        a.nx = nx;
        a.k = k;
        a.les = les;
        a.nut = nu_t;
        a.art = art;
        a.cles = cles;
        CFD_CHECK_HIP(pred_rows_launch<T>(a, use_supg != 0, tau_mode, vec, tuning().pred_rows, s));
        set_last_predictor(1, tau_mode, vec);
    } else {
        const dim3 grid = grid2d(ny, nx), block(256);
        if (les) {
            // the stand-alone nu_t pass, then nu_eff per cell from the stored nu_t
            hipLaunchKernelGGL(k_smagorinsky<T>, grid, block, 0, s, u, v, nu_t, ny, nx, cles, k);
            if (use_supg)
                hipLaunchKernelGGL((k_predictor<T, true, true>), grid, block, 0, s, u, v, (const T *)nu_t, nu_s,
                                   u_star, v_star, tau, ny, nx, dt, k, art);
            else
                hipLaunchKernelGGL((k_predictor<T, false, true>), grid, block, 0, s, u, v, (const T *)nu_t, nu_s,
                                   u_star, v_star, tau, ny, nx, dt, k, art);
        } else if (use_supg) {
            hipLaunchKernelGGL((k_predictor<T, true, false>), grid, block, 0, s, u, v, nu_eff, nu_s, u_star, v_star,
                               tau, ny, nx, dt, k, T(0));
        } else {
            hipLaunchKernelGGL((k_predictor<T, false, false>), grid, block, 0, s, u, v, nu_eff, nu_s, u_star, v_star,
                               tau, ny, nx, dt, k, T(0));
        }
        set_last_predictor(0, kTauExact, 1);
    }
    timing_end(tk, s, 1);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int divergence2d(const char *who, const T *u, const T *v, T *div, int ny, int nx, double dx, double dy, T *absmax,
                 void *stream) {
    CFD_REQUIRE(u && v && div, "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_divergence<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), u, v, div, ny, nx,
                       (T)(0.5 / dx), (T)(0.5 / dy), absmax);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int gradient2d(const char *who, const T *phi, T *grad_x, T *grad_y, int ny, int nx, double dx, double dy,
               void *stream) {
    CFD_REQUIRE(phi && grad_x && grad_y, "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_gradient<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), phi, grad_x, grad_y, ny, nx,
                       (T)(0.5 / dx), (T)(0.5 / dy));
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int project2d(const char *who, const T *phi, const T *u_star, const T *v_star, T *u, T *v, int ny, int nx, double dx,
              double dy, T dt, T *gradmax, void *stream) {
    CFD_REQUIRE(phi && u_star && v_star && u && v, "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_project<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), phi, u_star, v_star, u, v, ny,
                       nx, (T)(0.5 / dx), (T)(0.5 / dy), dt, gradmax);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

// clean_divergence_fast (v5.py:239-257) on row-major scratch fields phi and
// div in ws, `iterations` times: divergence, the plain lexicographic sweep,
// u -= dphi/dx, v -= dphi/dy.  phi starts at 0 (np.zeros_like, v5.py:242).
template <typename T>
int clean_divergence_plain(T *u, T *v, int ny, int nx, double dx, double dy, int iterations, void *ws,
                           hipStream_t s) {
    const size_t n = (size_t)ny * nx;
    T *phi = reinterpret_cast<T *>(ws);
    T *div = phi + n;
    CFD_CHECK_HIP(hipMemsetAsync(phi, 0, n * sizeof(T), s));
    const double dx2_inv = 1.0 / (dx * dx), dy2_inv = 1.0 / (dy * dy);
    const double denom_inv = 1.0 / (2.0 * (dx2_inv + dy2_inv));
    const T cx = (T)(0.5 / dx), cy = (T)(0.5 / dy);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_divergence<T>, grid2d(ny, nx), dim3(256), 0, s, u, v, div, ny, nx, cx, cy,
                           (T *)nullptr);
        if (ny > 2 && nx > 2)
            hipLaunchKernelGGL(k_lex_gs_sweep<T>, dim3(1), dim3(ny - 2 >= 1024 ? 1024 : 64 * ceil_div(ny - 2, 64)),
                               0, s, phi, div, ny, nx, (T)dx2_inv, (T)dy2_inv, (T)denom_inv);
        hipLaunchKernelGGL(k_sub_gradient<T>, grid2d(ny, nx), dim3(256), 0, s, phi, u, v, ny, nx, cx, cy);
        CFD_LAUNCH_CHECK();
    }
    return CFD_OK;
}

template <typename T>
int apply_bc2d(const char *who, T *u, T *v, const double *y, int ny, int nx, double y_max, double v_inf, int step,
               void *stream) {
    CFD_REQUIRE(u && v && y, "%s: null pointer", who);
    CFD_REQUIRE(ny >= 2 && nx >= 2, "%s: grid must be at least 2x2", who);
    const int n = ny > nx ? ny : nx;
    hipLaunchKernelGGL(k_bc<T>, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream), u, v, y, ny, nx, y_max,
                       v_inf, step);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int apply_lid_bc2d(const char *who, T *u, T *v, int ny, int nx, T u_lid, void *stream) {
    CFD_REQUIRE(u && v, "%s: null pointer", who);
    CFD_REQUIRE(ny >= 2 && nx >= 2, "%s: grid must be at least 2x2", who);
    const int n = ny > nx ? ny : nx;
    hipLaunchKernelGGL(k_lid_bc<T>, dim3(ceil_div(n, 256)), dim3(256), 0, as_stream(stream), u, v, ny, nx, u_lid);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int apply_ibm2d(const char *who, T *u, T *v, const double *ibm_mask, int n, double force_strength, void *stream) {
    CFD_REQUIRE(u && v && ibm_mask && n >= 0, "%s: bad arguments", who);
    if (n == 0) return CFD_OK;
    hipLaunchKernelGGL(k_ibm<T>, dim3(grid1d(n)), dim3(256), 0, as_stream(stream), u, v, ibm_mask, n,
                       force_strength);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int apply_bc_ibm2d(const char *who, T *u, T *v, const double *y, int ny, int nx, double y_max, double v_inf, int step,
                   const double *ibm_mask, double force_strength, void *stream) {
    CFD_REQUIRE(u && v && y, "%s: null pointer", who);
    CFD_REQUIRE(ny >= 2 && nx >= 2, "%s: grid must be at least 2x2", who);
    int blocks = ceil_div(ny > nx ? ny : nx, 256);
    if (ibm_mask) {
        const int g = grid1d((size_t)ny * nx);
        if (g > blocks) blocks = g;
    }
    hipLaunchKernelGGL(k_bc_ibm<T>, dim3(blocks), dim3(256), 0, as_stream(stream), u, v, y, ibm_mask, ny, nx, y_max,
                       v_inf, step, force_strength);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int clip_field(const char *who, T *a, size_t n, T lo, T hi, void *stream) {
    CFD_REQUIRE(a, "%s: null pointer", who);
    if (n == 0) return CFD_OK;
    hipLaunchKernelGGL(k_clip<T>, dim3(grid1d(n)), dim3(256), 0, as_stream(stream), a, n, lo, hi);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

// max |a| (and |b| when given) folded into *out
template <typename T>
int absmax2(const char *who, const T *a, const T *b, size_t n, T *out, void *stream) {
    CFD_REQUIRE(a && out, "%s: null pointer", who);
    if (n == 0) return CFD_OK;
    hipLaunchKernelGGL(k_absmax<T>, dim3(grid1d(n)), dim3(256), 0, as_stream(stream), a, b, n, out);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int mean_field(const char *who, const T *a, size_t n, double *out, void *stream) {
    CFD_REQUIRE(a && out && n > 0, "%s: bad arguments", who);
    hipStream_t s = as_stream(stream);
    unsigned *ws = energy_scratch(s);
    CFD_REQUIRE(ws, "%s: no scratch for the partial sums", who);
    hipLaunchKernelGGL(k_mean_mb<T>, dim3(kEnergyBlocks), dim3(256), 0, s, a, n, out, ws);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

// mean of 0.5 (u^2 + v^2); CLIP: then u, v <- clip(u, lo, hi), clip(v, lo, hi)
// (the step's two np.clip calls, v5.py:437-438), fused up to kEnergyOneBlock
template <typename T, bool CLIP>
int energy_mean2d(const char *who, T *u, T *v, size_t n, double *out, T lo, T hi, void *stream) {
    CFD_REQUIRE(u && v && out && n > 0, "%s: bad arguments", who);
    hipStream_t s = as_stream(stream);
    if (n <= kEnergyOneBlock) {
        if (unsigned *ws = energy_scratch(s))
            hipLaunchKernelGGL((k_energy_mean_mb<T, CLIP>), dim3(kEnergyBlocks), dim3(256), 0, s, u, v, n, out, lo, hi,
                               ws);
        else
            hipLaunchKernelGGL((k_energy_mean_1blk<T, CLIP>), dim3(1), dim3(1024), 0, s, u, v, n, out, lo, hi);
        CFD_LAUNCH_CHECK();
        return CFD_OK;
    }
    CFD_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(double), s));
    hipLaunchKernelGGL(k_energy_sum<T>, dim3(grid1d(n)), dim3(256), 0, s, (const T *)u, (const T *)v, n, out);
    hipLaunchKernelGGL(k_scale_double, dim3(1), dim3(1), 0, s, out, 1.0 / (double)n);
    CFD_LAUNCH_CHECK();
    if (!CLIP) return CFD_OK;
    const int rc = clip_field<T>(who, u, n, lo, hi, stream);
    return rc ? rc : clip_field<T>(who, v, n, lo, hi, stream);
}

// w (when given) and nanmax|w| folded into *absmax (when given)
template <typename T>
int vorticity2d(const char *who, const T *u, const T *v, const uint8_t *mask, T *w, T *absmax, int ny, int nx,
                double dx, double dy, void *stream) {
    CFD_REQUIRE(u && v && (w || absmax), "%s: null pointer", who);
    CFD_SHAPE2D(ny, nx);
    hipLaunchKernelGGL(k_vorticity<T>, grid2d(ny, nx), dim3(256), 0, as_stream(stream), u, v, mask, w, ny, nx,
                       (T)(2.0 * dx), (T)(2.0 * dy), absmax);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

template <typename T>
int nonfinite_count(const char *who, const T *a, const T *b, size_t n, int *out, void *stream) {
    CFD_REQUIRE(a && out, "%s: null pointer", who);
    hipStream_t s = as_stream(stream);
    CFD_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(int), s));
    if (n == 0) return CFD_OK;
    hipLaunchKernelGGL(k_nonfinite<T>, dim3(grid1d(n)), dim3(256), 0, s, a, b, n, out);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

}  // namespace cfd
