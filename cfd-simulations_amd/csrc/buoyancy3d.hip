// buoyancy3d.hip -- Boussinesq buoyancy in the 3-D fused predictor, for gfx950:
// the temperature of the 3-D cylinder channel acts back on the momentum,
//   f* = p + dt * (b_f * (T_C - t_ref)),   f in {u, v, w},
// with p what the plain predictor gives the interior cell (pred3_cell), T_C the
// cell's own incoming temperature and b = (bx, by, bz) the caller's float32
// coefficients (-Ri V_inf^2 / (D dT) along the gravity direction for the
// cylinder channel); the face cells keep f.  float32 operations in the order
// written, nothing fused; tests/buoyancy3d_reference.py states it as NumPy
// array code and the kernels reproduce it bit for bit.
//
// The term lives inside the predictor's kernels (BUOY of k_predictor3d_planes,
// pred_planes.hpp; the Pred3Buoy mode of k_predictor3d, fields3d.hip): one
// more 4-byte read per cell, no halo.  This file holds the plane march's
// buoyant instantiations -- cells per lane {1, 2, 4} x rows {1, 2} x SUPG x
// {scalar, LES} x {flat, periodic z}, every shape cfd_set_predictor3d_config
// can select -- and the four entry points; the checks and the dispatch are
// predictor3d_run's (fields3d.hip), the same as for the plain predictor.
#include "common.hpp"
#include "internal.hpp"
#include "pred_planes.hpp"

namespace cfd {

hipError_t pred_planes_launch_buoyant(const Pred3Args &a, bool supg, int nm, int vec, int rows, hipStream_t s,
                                      bool zper) {
    return pred_planes_launch<true>(a, supg, nm, vec, rows, 0, s, zper);
}

}  // namespace cfd

using namespace cfd;

extern "C" {

int cfd_predictor3d_buoy_f32(const float *u, const float *v, const float *w, const float *T, float nu_eff, float bx,
                             float by, float bz, float t_ref, float *u_star, float *v_star, float *w_star,
                             float *tau, int nz, int ny, int nx, double dx, double dy, double dz, float dt,
                             int use_supg, void *stream) {
    const Pred3Buoy b = {T, bx, by, bz, t_ref};
    return predictor3d_run("predictor3d_buoy", kNu3Scalar, false, u, v, w, nu_eff, nullptr, 0.0f, 0.0, u_star, v_star,
                           w_star, tau, nullptr, nz, ny, nx, dx, dy, dz, dt, use_supg, stream, &b);
}

int cfd_predictor3d_les_buoy_f32(const float *u, const float *v, const float *w, const float *T, float nu,
                                 float art_visc, double cs, float bx, float by, float bz, float t_ref, float *u_star,
                                 float *v_star, float *w_star, float *tau, float *nu_t, int nz, int ny, int nx,
                                 double dx, double dy, double dz, float dt, int use_supg, void *stream) {
    const Pred3Buoy b = {T, bx, by, bz, t_ref};
    return predictor3d_run("predictor3d_les_buoy", kNu3Les, false, u, v, w, nu, nullptr, art_visc, cs, u_star, v_star,
                           w_star, tau, nu_t, nz, ny, nx, dx, dy, dz, dt, use_supg, stream, &b);
}

int cfd_predictor3d_buoy_zper_f32(const float *u, const float *v, const float *w, const float *T, float nu_eff,
                                  float bx, float by, float bz, float t_ref, float *u_star, float *v_star,
                                  float *w_star, float *tau, int nz, int ny, int nx, double dx, double dy, double dz,
                                  float dt, int use_supg, void *stream) {
    const Pred3Buoy b = {T, bx, by, bz, t_ref};
    return predictor3d_run("predictor3d_buoy_zper", kNu3Scalar, true, u, v, w, nu_eff, nullptr, 0.0f, 0.0, u_star,
                           v_star, w_star, tau, nullptr, nz, ny, nx, dx, dy, dz, dt, use_supg, stream, &b);
}

int cfd_predictor3d_les_buoy_zper_f32(const float *u, const float *v, const float *w, const float *T, float nu,
                                      float art_visc, double cs, float bx, float by, float bz, float t_ref,
                                      float *u_star, float *v_star, float *w_star, float *tau, float *nu_t, int nz,
                                      int ny, int nx, double dx, double dy, double dz, float dt, int use_supg,
                                      void *stream) {
    const Pred3Buoy b = {T, bx, by, bz, t_ref};
    return predictor3d_run("predictor3d_les_buoy_zper", kNu3Les, true, u, v, w, nu, nullptr, art_visc, cs, u_star,
                           v_star, w_star, tau, nu_t, nz, ny, nx, dx, dy, dz, dt, use_supg, stream, &b);
}

}  // extern "C"
