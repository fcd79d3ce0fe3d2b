// scalar_planes.hpp -- the plane march of the passive scalar's advance
// (cfd_scalar_advance3d_f32): T_new = T + dt * (-conv + lap) with the
// predictor's per-cell arithmetic (pred3_cell / pred3_tau of pred_planes.hpp,
// unchanged) applied to T, advected by the cell's own (u, v, w), the cell's
// diffusivity ae in place of nu.
//
// The march is the predictor's (pred_planes.hpp: one wave owns 64 * VEC columns
// and R rows and marches along z through a chunk of planes; four waves of a
// workgroup stacked in y; per-plane buffer resources with 64-bit bases; the
// chunk-window test on the unwrapped plane index and the index modulo nz under
// ZPER; DPP x-neighbours with the segment's halo cell as `old`; streaming
// stores; no LDS, no barrier), with one difference that sets its traffic:
// only T is a stencil operand.  Of T the wave keeps the R own rows of plane
// k - 1, rows j0 - 1 .. j0 + R with the x-halo cells of plane k, the same of
// plane k + 1, and plane k + 2 in flight.  Of u, v, w (and nu_t) it keeps the
// R own rows of plane k alone, loaded one plane ahead: no halo rows, no halo
// cells, no neighbour planes.  So the model is 4 B read of each of T, u, v, w
// and 4 B written per cell, 20 B (24 B with nu_t), against the predictor's
// 24 B with three stencil fields.
#pragma once
#include "pred_planes.hpp"

namespace cfd {

struct Scalar3Args {
    const float *T, *u, *v, *w;
    const float *nut;  // NUT: nu_t per cell, ae = alpha + nu_t * inv_prt
    float *Tn;
    float alpha, inv_prt, dt;
    int nz, ny, nx;
    int zchunk, nseg, ntile;  // planes per chunk, segments per row, row tiles (4 waves x R rows)
    PredK3 k;
};

template <int VEC, int R, bool SUPG, bool NUT, bool ZPER>
__global__ __launch_bounds__(256) void k_scalar_advance3d_planes(Scalar3Args a) {
    constexpr int SW = 64 * VEC;  // segment width (columns)
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = xcd_swizzle((int)blockIdx.x, (int)gridDim.x);
    const int seg = b % a.nseg;
    const int bt = b / a.nseg;
    const int tile = bt % a.ntile;
    const int zc = bt / a.ntile;
    const int nz = a.nz, ny = a.ny, nx = a.nx;
    const int j0 = (tile * 4 + wv) * R;
    if (j0 >= ny) return;  // wave-uniform (no barrier in this kernel)
    const int z0 = zc * a.zchunk;
    const int z1 = min(z0 + a.zchunk, nz);
    const int xs = seg * SW;
    const int x0 = xs + lane * VEC;
    const bool lane_in = x0 < nx;  // nx % VEC == 0: a lane's cells are all in or all out
    const size_t plane = (size_t)ny * nx;
    const int pbytes = (int)(plane * sizeof(float));  // < 2^31 (checked by the launcher)
    // byte offset of this lane's cells in row j of a plane (kOob outside: reads 0, stores dropped)
    auto rofs = [&](int j) -> uint32_t {
        return ((j >= 0) & (j < ny) & lane_in) ? (uint32_t)(((size_t)j * nx + x0) * sizeof(float)) : kOob;
    };
    // the segment's x-halo cells of row j: lane 0 column xs - 1, lane 63 column xs + SW
    const int hx = lane == 0 ? xs - 1 : (lane == kWave - 1 ? xs + SW : -1);
    const bool h_in = hx >= 0 && hx < nx;
    auto hofs = [&](int j) -> uint32_t {
        return ((j >= 0) & (j < ny) & h_in) ? (uint32_t)(((size_t)j * nx + hx) * sizeof(float)) : kOob;
    };
    uint32_t ro[R + 2], ho[R];
#pragma unroll
    for (int r = 0; r < R + 2; ++r) ro[r] = rofs(j0 - 1 + r);
#pragma unroll
    for (int r = 0; r < R; ++r) ho[r] = hofs(j0 + r);
    // plane z of a field as a buffer resource: an empty range (reads 0) when
    // not wanted or outside [max(z0 - 1, 0), min(z1, nz - 1)] (ZPER: the
    // window [z0 - 1, z1] on the unwrapped index, then the index modulo nz)
    const int zlo = ZPER ? z0 - 1 : max(z0 - 1, 0), zhi = ZPER ? z1 : min(z1, nz - 1);
    auto prsrc = [&](const float *base, int z, bool want) {
        const bool in = want && z >= zlo && z <= zhi;
        if constexpr (ZPER) z = z < 0 ? z + nz : (z >= nz ? z - nz : z);  // -1 .. nz only (the window)
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base) + (in ? (size_t)z * plane : 0), 0,
                                                 in ? pbytes : 0, 0x00020000);
    };
    auto load_plane = [&](int z) {
        const __amdgpu_buffer_rsrc_t rs = prsrc(a.T, z, true);
        Plane<VEC, R> p;
#pragma unroll
        for (int r = 0; r < R + 2; ++r) p.row[r] = pldv<float, VEC>(rs, ro[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) p.halo[r] = pld1<float>(rs, ho[r]);
        return p;
    };
    // the R own rows of plane z of an advecting field (want: z inside the chunk)
    auto load_own = [&](const float *base, int z, bool want, Cells<float, VEC> (&dst)[R]) {
        const __amdgpu_buffer_rsrc_t rs = prsrc(base, z, want);
#pragma unroll
        for (int r = 0; r < R; ++r) dst[r] = pldv<float, VEC>(rs, ro[r + 1]);
    };
    const float dt = a.dt, alpha = a.alpha;

    Cells<float, VEC> Tm[R];  // plane k - 1, own rows
    load_own(a.T, z0 - 1, true, Tm);
    Plane<VEC, R> Tc = load_plane(z0), Tp = load_plane(z0 + 1);
    Cells<float, VEC> Uc[R], Vc[R], Wc[R];
    [[maybe_unused]] Cells<float, VEC> Nc[R];
    load_own(a.u, z0, true, Uc);
    load_own(a.v, z0, true, Vc);
    load_own(a.w, z0, true, Wc);
    if constexpr (NUT) load_own(a.nut, z0, true, Nc);
    for (int z = z0; z < z1; ++z) {
        // the advecting fields one plane ahead, T two planes ahead
        Cells<float, VEC> Un[R], Vn[R], Wn[R];
        [[maybe_unused]] Cells<float, VEC> Nn[R];
        const bool more = z + 1 < z1;
        load_own(a.u, z + 1, more, Un);
        load_own(a.v, z + 1, more, Vn);
        load_own(a.w, z + 1, more, Wn);
        if constexpr (NUT) load_own(a.nut, z + 1, more, Nn);
        const Plane<VEC, R> Tn = load_plane(z + 2);
        const bool zin = ZPER || (z >= 1 && z <= nz - 2);  // wave-uniform
        const __amdgpu_buffer_rsrc_t rout =
            __builtin_amdgcn_make_buffer_rsrc(a.Tn + (size_t)z * plane, 0, pbytes, 0x00020000);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = j0 + r;
            Cells<float, VEC> o = Tc.row[r + 1];  // the faces keep T
            if (zin && j >= 1 && j <= ny - 2) {   // wave-uniform
                const float *tc = Tc.row[r + 1].x;
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    Nb7 f;
                    f.C = tc[c];
                    f.E = c < VEC - 1 ? tc[c + 1] : dpp_from_upper_old(Tc.halo[r], tc[0]);
                    f.W = c > 0 ? tc[c - 1] : dpp_from_lower_old(Tc.halo[r], tc[VEC - 1]);
                    f.N = Tc.row[r + 2].x[c];
                    f.S = Tc.row[r].x[c];
                    f.U = Tp.row[r + 1].x[c];
                    f.D = Tm[r].x[c];
                    const float uc = Uc[r].x[c], vc = Vc[r].x[c], wc = Wc[r].x[c];
                    float ae = alpha;  // the cell's diffusivity
                    if constexpr (NUT) ae = alpha + Nc[r].x[c] * a.inv_prt;
                    float t = 0.0f;
                    if constexpr (SUPG) t = pred3_tau(uc, vc, wc, ae, dt, a.k);
                    const float tn = pred3_cell<SUPG>(uc, vc, wc, f, t, ae, dt, a.k);
                    const bool in = x0 + c >= 1 && x0 + c <= nx - 2;
                    o.x[c] = in ? tn : tc[c];
                }
            }
            pstv<float, VEC>(o, rout, ro[r + 1]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            Tm[r] = Tc.row[r + 1];
            Uc[r] = Un[r];
            Vc[r] = Vn[r];
            Wc[r] = Wn[r];
            if constexpr (NUT) Nc[r] = Nn[r];
        }
        Tc = Tp;
        Tp = Tn;
    }
}

template <int VEC, int R, bool ZPER>
inline const void *scalar_planes_kernel(bool supg, bool nut) {
    if (supg)
        return nut ? (const void *)k_scalar_advance3d_planes<VEC, R, true, true, ZPER>
                   : (const void *)k_scalar_advance3d_planes<VEC, R, true, false, ZPER>;
    return nut ? (const void *)k_scalar_advance3d_planes<VEC, R, false, true, ZPER>
               : (const void *)k_scalar_advance3d_planes<VEC, R, false, false, ZPER>;
}
template <int VEC, int R>
inline const void *scalar_planes_kernel(bool supg, bool nut, bool zper) {
    return zper ? scalar_planes_kernel<VEC, R, true>(supg, nut) : scalar_planes_kernel<VEC, R, false>(supg, nut);
}

// Plane-march launch: cells per lane vec (1, 2, 4), rows per wave rows (1, 2),
// planes per chunk zchunk (0: the predictor's auto rule); a.nseg / a.ntile /
// a.zchunk are filled here.  The caller has checked shape (a plane below 2^31
// bytes, nx % vec == 0) and alignment.
inline hipError_t scalar_planes_launch(Scalar3Args a, bool supg, bool zper, int vec, int rows, int zchunk,
                                       hipStream_t s) {
    const bool nut = a.nut != nullptr;
    const void *f;
    if (rows == 1)
        f = vec == 4   ? scalar_planes_kernel<4, 1>(supg, nut, zper)
            : vec == 2 ? scalar_planes_kernel<2, 1>(supg, nut, zper)
                       : scalar_planes_kernel<1, 1>(supg, nut, zper);
    else
        f = vec == 4   ? scalar_planes_kernel<4, 2>(supg, nut, zper)
            : vec == 2 ? scalar_planes_kernel<2, 2>(supg, nut, zper)
                       : scalar_planes_kernel<1, 2>(supg, nut, zper);
    a.nseg = ceil_div(a.nx, 64 * vec);
    a.ntile = ceil_div(a.ny, 4 * rows);
    a.zchunk = zchunk;
    if (a.zchunk <= 0) {  // each chunk re-reads 2 planes of T: 8 .. 32 planes, ~2048 workgroups where the grid has them
        const long per = (long)a.nseg * a.ntile;
        long zcn = ((long)a.nz * per) / 2048;
        a.zchunk = (int)(zcn < 8 ? 8 : (zcn > 32 ? 32 : zcn));
    }
    const long nblk = (long)a.nseg * a.ntile * ceil_div(a.nz, a.zchunk);
    if (nblk > 0x7fffffffL) return hipErrorInvalidValue;
    void *args[] = {&a};
    return hipLaunchKernel(f, dim3((unsigned)nblk), dim3(256), args, 0, s);
}

}  // namespace cfd
