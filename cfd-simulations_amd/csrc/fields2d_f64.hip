// fields2d_f64.hip -- the time_step() kernels with float64 fields
// (memory_efficient=False, v5.py:287-296): every field array is float64 and
// the dtype-generic @njit kernels (v5.py:96-257) run in float64.  The
// one-thread-per-cell kernels and their launchers are the double
// instantiations of fields2d_cells.hpp.
//
// Arithmetic, as the reference executes it under NumPy 2 (NEP 50): Python
// float constants stay float64 against float64 data (no rounding to float32,
// unlike fields2d.hip).  The step's dt is np.float32 (adaptive_time_step) or
// the Python float dt_base (adaptive_dt=False, v5.py:317-318); either way it
// meets the float64 fields exactly, so the entry points take it as a double
// (tau = dt / 2, v5.py:161, is then exact in both precisions).  The GS's
// dt_inv = 1.0 / cfg.dt is a float32 quotient (cfg.dt is np.float32, v5.py:210).
// Source operation order, nothing fused (-ffp-contract=off).
//
// The SUPG tau's |V| = (u**2 + v**2) ** 0.5 on float64 scalars goes through
// glibc's pow in the reference, which is not correctly rounded; it runs here
// as the device restatement of that pow (vel_mag, fields2d_cells.hpp), so the
// float64 step is bit-exact against the reference's own steps like the
// float32 one.
//
// The float64 path is the reference's secondary configuration (every
// reference script sets memory_efficient=True, v5.py:633): clean_divergence
// takes the plain lexicographic sweep at every size, and the red-black GS
// runs as in-place colour passes, two launches per iteration, with the
// device-side stop rule of the float32 path.
#include "fields2d_cells.hpp"

namespace cfd {
namespace {

// ------------------------------------------------------ red-black GS, fp64
// Workspace (cfd_rbgs_workspace_bytes): int flags[4] (iterations, done,
// unused, unused), then double maxc[iterations] at byte 16.
struct RbgsWs64 {
    int flags[4];
    double maxc[1];
};

__global__ void k_rbgs64_init(RbgsWs64 *ws, int iterations, int *iters_done) {
    for (int k = threadIdx.x; k < iterations; k += blockDim.x) ws->maxc[k] = 0.0;
    if (threadIdx.x == 0) {
        ws->flags[0] = iterations;
        ws->flags[1] = iterations;
        ws->flags[2] = ws->flags[3] = 0;
        if (iters_done) *iters_done = iterations;
    }
}

// One colour of iteration `it`, in place, v5.py:211-222: colour c visits
// j = 1 + (i + c) % 2 step 2, masked cells skipped; max|change| into maxc[it].
// Skipped once an earlier iteration ended below tol (v5.py:224-225; maxc of
// skipped iterations stays 0 < tol, so the stop persists).
template <int C>
__global__ __launch_bounds__(256) void k_rbgs64_color(double *__restrict__ phi, const double *__restrict__ div,
                                                      const uint8_t *__restrict__ mask, int ny, int nx, double cx,
                                                      double cy, double cd, double dt_inv, double tol,
                                                      RbgsWs64 *ws, int it) {
    if (it > 0 && ws->maxc[it - 1] < tol) return;
    const int i = blockIdx.y + 1;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    double mx = 0.0;
    if (j >= 1 && j < nx - 1 && ((i + j + 1 + C) & 1) == 0) {
        const size_t c = (size_t)i * nx + j;
        if (!(mask && mask[c])) {
            const double rhs = -div[c] * dt_inv;
            const double pn = (cx * (phi[c + 1] + phi[c - 1]) + cy * (phi[c + nx] + phi[c - nx]) - rhs) * cd;
            const double ch = fabs(pn - phi[c]);
            if (ch > mx) mx = ch;
            phi[c] = pn;
        }
    }
    wave_reduce_max_store(mx, &ws->maxc[it]);
}

// iterations done = 1 + the first iteration whose max|change| < tol, else all
__global__ void k_rbgs64_count(RbgsWs64 *__restrict__ ws, double tol, int *iters_done) {
    const int n = ws->flags[0];
    int first = n;
    for (int base = 0; base < n; base += 64) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long m = __ballot(i < n && ws->maxc[i] < tol);
        if (m) {
            first = base + __ffsll((long long)m) - 1;
            break;
        }
    }
    if (threadIdx.x == 0) {
        const int c = first < n ? first + 1 : n;
        ws->flags[1] = c;
        if (iters_done) *iters_done = c;
    }
}

}  // namespace
}  // namespace cfd

using namespace cfd;

// NumPy float64 scalar power (glibc pow, libm_pow.hpp) elementwise: the
// parity hook for the device pow the float64 SUPG tau uses.
__global__ void k_numpy_pow64(const double *__restrict__ x, double y, double *__restrict__ out, size_t n) {
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x)
        out[c] = libm::pow(x[c], y);
}

extern "C" {

int cfd_supg_tau2d_f64(const double *u, const double *v, const double *nu_eff, double nu_eff_scalar, double *tau,
                       int ny, int nx, double dx, double dy, double dt, void *stream) {
    return supg_tau2d<double>("supg_tau2d_f64", u, v, nu_eff, nu_eff_scalar, tau, ny, nx, dx, dy, dt, stream);
}

int cfd_convection_supg2d_f64(const double *u, const double *v, const double *phi, const double *tau,
                              double *conv, int ny, int nx, double dx, double dy, void *stream) {
    return convection_supg2d<double>("convection_supg2d_f64", u, v, phi, tau, conv, ny, nx, dx, dy, stream);
}

int cfd_convection_upwind2d_f64(const double *u, const double *v, const double *phi, double *conv, int ny, int nx,
                                double dx, double dy, void *stream) {
    return convection_upwind2d<double>("convection_upwind2d_f64", u, v, phi, conv, ny, nx, dx, dy, stream);
}

int cfd_laplacian2d_f64(const double *phi, const double *nu_eff, double nu_eff_scalar, double *lap, int ny, int nx,
                        double dx, double dy, void *stream) {
    return laplacian2d<double>("laplacian2d_f64", phi, nu_eff, nu_eff_scalar, lap, ny, nx, dx, dy, stream);
}

int cfd_predictor2d_f64(const double *u, const double *v, const double *nu_eff, double nu_eff_scalar,
                        double *u_star, double *v_star, double *tau, int ny, int nx, double dx, double dy, double dt,
                        int use_supg, void *stream) {
    return predictor2d<double>("predictor2d_f64", u, v, nu_eff, nu_eff_scalar, u_star, v_star, tau, ny, nx, dx, dy,
                               dt, use_supg, stream, false, 0.0, 0.0, nullptr);
}

int cfd_predictor2d_les_f64(const double *u, const double *v, double nu, double art_visc, double cs, double *u_star,
                            double *v_star, double *tau, double *nu_t, int ny, int nx, double dx, double dy,
                            double dt, int use_supg, void *stream) {
    return predictor2d<double>("predictor2d_les_f64", u, v, nullptr, nu, u_star, v_star, tau, ny, nx, dx, dy, dt,
                               use_supg, stream, true, art_visc, cs, nu_t);
}

int cfd_smagorinsky2d_f64(const double *u, const double *v, double *nu_t, int ny, int nx, double dx, double dy,
                          double cs, void *stream) {
    return smagorinsky2d<double>("smagorinsky2d_f64", u, v, nu_t, ny, nx, dx, dy, cs, stream);
}

int cfd_mean_f64(const double *a, size_t n, double *out, void *stream) {
    return mean_field<double>("mean_f64", a, n, out, stream);
}

int cfd_divergence2d_f64(const double *u, const double *v, double *div, int ny, int nx, double dx, double dy,
                         double *absmax, void *stream) {
    return divergence2d<double>("divergence2d_f64", u, v, div, ny, nx, dx, dy, absmax, stream);
}

int cfd_gradient2d_f64(const double *phi, double *grad_x, double *grad_y, int ny, int nx, double dx, double dy,
                       void *stream) {
    return gradient2d<double>("gradient2d_f64", phi, grad_x, grad_y, ny, nx, dx, dy, stream);
}

int cfd_project2d_f64(const double *phi, const double *u_star, const double *v_star, double *u, double *v, int ny,
                      int nx, double dx, double dy, double dt, double *gradmax, void *stream) {
    return project2d<double>("project2d_f64", phi, u_star, v_star, u, v, ny, nx, dx, dy, dt, gradmax, stream);
}

int cfd_clean_divergence2d_f64(double *u, double *v, int ny, int nx, double dx, double dy, int iterations,
                               void *ws, void *stream) {
    CFD_REQUIRE(u && v && ws, "clean_divergence2d_f64: null pointer");
    CFD_SHAPE2D(ny, nx);
    return clean_divergence_plain<double>(u, v, ny, nx, dx, dy, iterations, ws, as_stream(stream));
}

int cfd_apply_bc2d_f64(double *u, double *v, const double *y, int ny, int nx, double y_max, double v_inf,
                       int step, void *stream) {
    return apply_bc2d<double>("apply_bc2d_f64", u, v, y, ny, nx, y_max, v_inf, step, stream);
}

int cfd_apply_lid_bc2d_f64(double *u, double *v, int ny, int nx, double u_lid, void *stream) {
    return apply_lid_bc2d<double>("apply_lid_bc2d_f64", u, v, ny, nx, u_lid, stream);
}

int cfd_apply_ibm2d_f64(double *u, double *v, const double *ibm_mask, int n, double force_strength,
                        void *stream) {
    return apply_ibm2d<double>("apply_ibm2d_f64", u, v, ibm_mask, n, force_strength, stream);
}

int cfd_numpy_pow_f64(const double *x, double y, double *out, size_t n, void *stream) {
    CFD_REQUIRE(x && out, "numpy_pow_f64: null pointer");
    if (n == 0) return CFD_OK;
    hipLaunchKernelGGL(k_numpy_pow64, dim3(grid1d(n)), dim3(256), 0, as_stream(stream), x, y, out, n);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_clip_f64(double *a, size_t n, double lo, double hi, void *stream) {
    return clip_field<double>("clip_f64", a, n, lo, hi, stream);
}

int cfd_absmax2_f64(const double *a, const double *b, size_t n, double *out, void *stream) {
    return absmax2<double>("absmax2_f64", a, b, n, out, stream);
}

int cfd_energy_mean2d_f64(const double *u, const double *v, size_t n, double *out, void *stream) {
    return energy_mean2d<double, false>("energy_mean2d_f64", const_cast<double *>(u), const_cast<double *>(v), n, out,
                                        0.0, 0.0, stream);
}

int cfd_energy_mean_clip2d_f64(double *u, double *v, size_t n, double *out, double lo, double hi, void *stream) {
    return energy_mean2d<double, true>("energy_mean_clip2d_f64", u, v, n, out, lo, hi, stream);
}

int cfd_apply_bc_ibm2d_f64(double *u, double *v, const double *y, int ny, int nx, double y_max, double v_inf, int step,
                           const double *ibm_mask, double force_strength, void *stream) {
    return apply_bc_ibm2d<double>("apply_bc_ibm2d_f64", u, v, y, ny, nx, y_max, v_inf, step, ibm_mask,
                                  force_strength, stream);
}

int cfd_vorticity2d_f64(const double *u, const double *v, const uint8_t *mask, double *w, double *absmax, int ny,
                        int nx, double dx, double dy, void *stream) {
    return vorticity2d<double>("vorticity2d_f64", u, v, mask, w, absmax, ny, nx, dx, dy, stream);
}

int cfd_nonfinite_count_f64(const double *a, const double *b, size_t n, int *out, void *stream) {
    return nonfinite_count<double>("nonfinite_count_f64", a, b, n, out, stream);
}

int cfd_rbgs2d_f64(double *phi, const double *div, const uint8_t *mask, int ny, int nx, double dx, double dy,
                   float dt, int iterations, double tolerance, void *ws, int *iters_done, void *stream) {
    CFD_REQUIRE(phi && div && ws, "rbgs2d_f64: null pointer");
    CFD_REQUIRE(ny >= 1 && nx >= 1 && iterations >= 0, "rbgs2d_f64: bad arguments");
    hipStream_t s = as_stream(stream);
    // v5.py:205-210: Python-float constants (float64 against float64 data);
    // dt_inv = 1.0 / np.float32(dt) is a float32 quotient
    const double dx2_inv = 1.0 / (dx * dx), dy2_inv = 1.0 / (dy * dy);
    const double denom_inv = 1.0 / (2.0 * (dx2_inv + dy2_inv));
    const double dt_inv = (double)(1.0f / dt);
    RbgsWs64 *w = reinterpret_cast<RbgsWs64 *>(ws);
    hipLaunchKernelGGL(k_rbgs64_init, dim3(1), dim3(1024), 0, s, w, iterations, iters_done);
    CFD_LAUNCH_CHECK();
    if (ny < 3 || nx < 3 || iterations == 0) return CFD_OK;
    const int tk = timing_begin(s);
    const dim3 grid(ceil_div(nx, 256), ny - 2);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_rbgs64_color<0>, grid, dim3(256), 0, s, phi, div, mask, ny, nx, dx2_inv, dy2_inv,
                           denom_inv, dt_inv, tolerance, w, it);
        hipLaunchKernelGGL(k_rbgs64_color<1>, grid, dim3(256), 0, s, phi, div, mask, ny, nx, dx2_inv, dy2_inv,
                           denom_inv, dt_inv, tolerance, w, it);
        CFD_LAUNCH_CHECK();
    }
    timing_end(tk, s, iterations);
    hipLaunchKernelGGL(k_rbgs64_count, dim3(1), dim3(64), 0, s, w, tolerance, iters_done);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

}  // extern "C"
