// pred_planes.hpp -- the 3-D fused advection-diffusion predictor: the project's
// own generalisation of the v5 templates (pred_rows.hpp) to (nz, ny, nx) fields
// u, v, w, every 2-D coefficient kept (the SUPG derivative factors 1/(4 dx),
// 1/(4 dx^2) included) and a z term appended to every sum.  The per-cell
// arithmetic below is shared by the one-thread-per-cell kernel (fields3d.hip)
// and the plane march, so the two give the same bits.
//
// Plane march.  One wave owns a segment of 64 * VEC columns (64 lanes x VEC
// adjacent cells) and R rows, and marches along z through a chunk of planes.
// Of each field it keeps in registers: the R rows of plane k - 1 (D), rows
// j0 - 1 .. j0 + R of planes k (centre, N / S) and k + 1 (U), and the same
// rows of plane k + 2 in flight -- every plane is loaded once per wave, two
// steps ahead.  x-neighbours are the lane's own cells plus DPP wave shifts;
// the two columns just outside the segment arrive as one load per row, field
// and plane (lane 0: column xs - 1, lane 63: column xs + 64 VEC) and enter the
// shifts as their `old` operand, as in the 2-D row march.  The y-halo rows
// (2 of R + 2 loaded rows) are rows another wave owns: the four waves of a
// workgroup are stacked in y and march the same planes together, so three of
// the four row pairs a workgroup re-reads were just loaded by a wave of the
// same CU, and the pair at the tile's edge by the workgroup dealt next
// (XCD-swizzled: the same L2).  No LDS: at R = 2, VEC = 4 the exchange would
// save 8 of 24 row loads per plane and field, all of them cache hits, for two
// barriers per plane.  u*, v*, w* and tau leave as streaming stores.
//
// Viscosity modes (NM).  kNu3Array: the cell's nu_eff is read from an array of
// the fields' shape -- the R own rows of its plane, loaded one plane ahead, no
// halo.  kNu3Les: the Smagorinsky nu_t of the cell (smag3_nut) is formed from
// values the march holds anyway -- E: the lane's next cell or the DPP shift
// with the halo cell as `old`, N: row[r + 2], U: the plane k + 1 -- so LES
// costs no extra read; nu_t is zeroed on the side columns by the `in`
// predicate (face rows and planes are wave-uniform) and leaves as a streaming
// store through its own per-plane buffer resource.  The scalar instantiations
// are unchanged by the other two modes (if constexpr throughout).
//
// Indexing is 64-bit: each plane gets its own buffer resource (base pointer
// advanced by k * ny * nx elements in 64 bits, one plane's bytes as the
// range), so offsets stay below 2^31 on arrays of any size; a plane outside
// the grid, or past the chunk's last U plane, gets an empty range and reads 0.
//
// ZPER (spanwise-periodic z): every plane is interior in z and the plane index
// of a resource is taken modulo nz -- the first chunk preloads plane nz - 1 as
// its D, the last chunk loads plane 0 as its U -- while the chunk-window test
// stays on the unwrapped index.  A template parameter: the non-periodic
// instantiations are the code they were.
//
// BUOY (Boussinesq buoyancy): f* gains dt * (b_f * (T_C - t_ref)) on the cells
// pred3_cell updates, with T_C the cell's own temperature: the R own rows of
// plane k of T, loaded one plane ahead, no halo -- kNu3Array's pattern, one
// more 4-byte read per cell.  Scalar and LES viscosity only (the solver has no
// array-nu step).  A template parameter: the instantiations without it are
// the code they were; the buoyant ones live in buoyancy3d.hip.
#pragma once
#include "common.hpp"
#include "pred_rows.hpp"

namespace cfd {

// stencil constants: make_pred_k plus the z analogues (formed in double,
// rounded once to float)
struct PredK3 {
    float c1x, c1y, c1z;  // SUPG first derivative: 0.5 * (0.5/dx)
    float c2x, c2y, c2z;  // SUPG second derivative: (0.5/dx)^2
    float ux, uy, uz;     // upwind: 1/dx
    float lx, ly, lz;     // laplacian: 1/(dx*dx)
    float h;              // min(dx, dy, dz)
    float eps;            // 1e-10
};
inline PredK3 make_pred_k3(double dx, double dy, double dz) {
    PredK3 k;
    const double sdx = 0.5 / dx, sdy = 0.5 / dy, sdz = 0.5 / dz;
    k.c1x = (float)(0.5 * sdx);
    k.c1y = (float)(0.5 * sdy);
    k.c1z = (float)(0.5 * sdz);
    k.c2x = (float)(sdx * sdx);
    k.c2y = (float)(sdy * sdy);
    k.c2z = (float)(sdz * sdz);
    k.ux = (float)(1.0 / dx);
    k.uy = (float)(1.0 / dy);
    k.uz = (float)(1.0 / dz);
    k.lx = (float)(1.0 / (dx * dx));
    k.ly = (float)(1.0 / (dy * dy));
    k.lz = (float)(1.0 / (dz * dz));
    const double hxy = dx < dy ? dx : dy;
    k.h = (float)(hxy < dz ? hxy : dz);
    k.eps = (float)1e-10;
    return k;
}

// SUPG tau of one interior cell: |V| = sqrt((u*u + v*v) + w*w) correctly
// rounded, then supg_tau_vm (IEEE divisions)
__device__ inline float pred3_tau(float u, float v, float w, float nu, float dt, const PredK3 &k) {
    PredK<float> k2 = {};
    k2.h = k.h;
    k2.eps = k.eps;
    const float vm = sqrt_ieee((u * u + v * v) + w * w);
    return supg_tau_vm(vm, nu, dt, k2);
}

// one field's centre value and six neighbours (E/W = x+-1, N/S = y+-1, U/D = z+-1)
struct Nb7 {
    float C, E, W, N, S, U, D;
};

// Viscosity of the predictor: one scalar for every cell (kNu3Scalar), an
// array of the fields' shape read per cell (kNu3Array), or LES (kNu3Les):
// the Smagorinsky nu_t of the cell formed from values the kernel holds anyway,
// then nu_eff = (nu + nu_t) + art_visc per cell.
enum { kNu3Scalar = 0, kNu3Array = 1, kNu3Les = 2 };

// The project's own 3-D form of compute_smagorinsky_viscosity_fast (the
// reference is 2-D and ships with LES off; tests/les3d_reference.py states
// this arithmetic): forward differences of u, v, w to the east, north and up
// neighbours, q = 2 (ux^2 + vy^2 + wz^2) + (uy + vx)^2 + (uz + wx)^2 +
// (vz + wy)^2 in the order below, nu_t = c2 sqrt(q) with the sqrt correctly
// rounded; c2 = float(smag3_const).  One interior cell.
__device__ inline float smag3_nut(const Nb7 &u, const Nb7 &v, const Nb7 &w, float c2, const PredK3 &k) {
    const float dux = (u.E - u.C) * k.ux, duy = (u.N - u.C) * k.uy, duz = (u.U - u.C) * k.uz;
    const float dvx = (v.E - v.C) * k.ux, dvy = (v.N - v.C) * k.uy, dvz = (v.U - v.C) * k.uz;
    const float dwx = (w.E - w.C) * k.ux, dwy = (w.N - w.C) * k.uy, dwz = (w.U - w.C) * k.uz;
    const float d = (dux * dux + dvy * dvy) + dwz * dwz;
    const float sxy = duy + dvx, sxz = duz + dwx, syz = dvz + dwy;
    const float o = (sxy * sxy + sxz * sxz) + syz * syz;
    const float q = 2.0f * d + o;
    return c2 * sqrt_ieee(q);
}
// (cs * (dx*dy*dz) ** (1.0/3.0)) ** 2 in Python floats: both `**` are libm's
// pow (exponents kept opaque, as in smag_const); the caller rounds it to float
inline double smag3_const(double cs, double dx, double dy, double dz) {
    volatile double third = 1.0 / 3.0, two = 2.0;
    return std::pow(cs * std::pow(dx * dy * dz, third), two);
}

// f* = f + dt * (-conv + lap) of one interior cell of field f (uc, vc, wc: the
// centre velocities; t: the cell's tau, SUPG only)
template <bool SUPG>
__device__ inline float pred3_cell(float uc, float vc, float wc, const Nb7 &f, float t, float nu, float dt,
                                   const PredK3 &k) {
    // the second differences, shared by SUPG and the Laplacian
    const float x2 = (f.E - 2.0f * f.C) + f.W;
    const float y2 = (f.N - 2.0f * f.C) + f.S;
    const float z2 = (f.U - 2.0f * f.C) + f.D;
    float conv;
    if constexpr (SUPG) {
        const float ddx = (f.E - f.W) * k.c1x;
        const float ddy = (f.N - f.S) * k.c1y;
        const float ddz = (f.U - f.D) * k.c1z;
        const float cs = (uc * ddx + vc * ddy) + wc * ddz;
        const float d2x = x2 * k.c2x, d2y = y2 * k.c2y, d2z = z2 * k.c2z;
        const float cd = cs - t * ((uc * d2x + vc * d2y) + wc * d2z);
        conv = t > 0.0f ? cd : cs;
    } else {
        const float ddx = uc > 0.0f ? (f.C - f.W) * k.ux : (f.E - f.C) * k.ux;
        const float ddy = vc > 0.0f ? (f.C - f.S) * k.uy : (f.N - f.C) * k.uy;
        const float ddz = wc > 0.0f ? (f.C - f.D) * k.uz : (f.U - f.C) * k.uz;
        conv = (uc * ddx + vc * ddy) + wc * ddz;
    }
    const float l1 = x2 * k.lx, l2 = y2 * k.ly, l3 = z2 * k.lz;
    const float lap = nu * ((l1 + l2) + l3);
    return f.C + dt * (-conv + lap);
}

struct Pred3Args {
    const float *u, *v, *w;
    float *us, *vs, *ws, *tau;  // tau: null = not written
    float nu, dt;
    int nz, ny, nx;
    int zchunk, nseg, ntile;  // planes per chunk, segments per row, row tiles (4 waves x R rows)
    PredK3 k;
    // kNu3Array: nu_eff per cell.  kNu3Les: nu_eff = (nu + nu_t) + art with
    // nu_t = c2 sqrt(q) (smag3_nut); nut: null = not written
    const float *nu_arr;
    float *nut;
    float c2, art;
    // BUOY: f* += dt * (b_f * (T - t_ref)) on the interior; T: the step's incoming temperature
    const float *T;
    float bx, by, bz, t_ref;
};

// the buoyant term's arguments as the per-cell kernel and the launchers take them
struct Pred3Buoy {
    const float *T;
    float bx, by, bz, t_ref;
};

// rows j0 - 1 .. j0 + R of one plane of one field (index 0 = row j0 - 1) and
// the segment's x-halo cells of rows j0 .. j0 + R - 1
template <int VEC, int R>
struct Plane {
    Cells<float, VEC> row[R + 2];
    float halo[R];
};

template <int VEC, int R, bool SUPG, int NM = kNu3Scalar, bool ZPER = false, bool BUOY = false>
__global__ __launch_bounds__(256) void k_predictor3d_planes(Pred3Args a) {
    static_assert(!ZPER || NM != kNu3Array, "periodic z: scalar and LES viscosity only");
    static_assert(!BUOY || NM != kNu3Array, "buoyancy: scalar and LES viscosity only");
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
    // plane z of a field as a buffer resource: an empty range outside
    // [max(z0 - 1, 0), min(z1, nz - 1)] (nothing there is ever used)
    auto prsrc = [&](const float *base, int z) {
        const bool in = (ZPER || (z >= 0 && z < nz)) && z >= z0 - 1 && z <= z1;
        if constexpr (ZPER) z = z < 0 ? z + nz : (z >= nz ? z - nz : z);  // -1 .. nz only (the window)
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base) + (in ? (size_t)z * plane : 0), 0,
                                                 in ? pbytes : 0, 0x00020000);
    };
    auto load_plane = [&](const float *base, int z) {
        const __amdgpu_buffer_rsrc_t rs = prsrc(base, z);
        Plane<VEC, R> p;
#pragma unroll
        for (int r = 0; r < R + 2; ++r) p.row[r] = pldv<float, VEC>(rs, ro[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) p.halo[r] = pld1<float>(rs, ho[r]);
        return p;
    };
    const float dt = a.dt, nu = a.nu;

    // plane k - 1 (its R own rows), k, k + 1 and k + 2 (in flight) of u, v, w
    Cells<float, VEC> Um[R], Vm[R], Wm[R];
    {
        const __amdgpu_buffer_rsrc_t r0 = prsrc(a.u, z0 - 1), r1 = prsrc(a.v, z0 - 1), r2 = prsrc(a.w, z0 - 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            Um[r] = pldv<float, VEC>(r0, ro[r + 1]);
            Vm[r] = pldv<float, VEC>(r1, ro[r + 1]);
            Wm[r] = pldv<float, VEC>(r2, ro[r + 1]);
        }
    }
    Plane<VEC, R> Uc = load_plane(a.u, z0), Vc = load_plane(a.v, z0), Wc = load_plane(a.w, z0);
    Plane<VEC, R> Up = load_plane(a.u, z0 + 1), Vp = load_plane(a.v, z0 + 1), Wp = load_plane(a.w, z0 + 1);
    // kNu3Array: the R own rows of nu_eff, one plane ahead (no halo)
    [[maybe_unused]] Cells<float, VEC> Nc[R];
    if constexpr (NM == kNu3Array) {
        const __amdgpu_buffer_rsrc_t rn = prsrc(a.nu_arr, z0);
#pragma unroll
        for (int r = 0; r < R; ++r) Nc[r] = pldv<float, VEC>(rn, ro[r + 1]);
    }
    // BUOY: the R own rows of T, one plane ahead (no halo)
    [[maybe_unused]] Cells<float, VEC> Tc[R];
    if constexpr (BUOY) {
        const __amdgpu_buffer_rsrc_t rt0 = prsrc(a.T, z0);
#pragma unroll
        for (int r = 0; r < R; ++r) Tc[r] = pldv<float, VEC>(rt0, ro[r + 1]);
    }
    for (int z = z0; z < z1; ++z) {
        [[maybe_unused]] Cells<float, VEC> Nn[R];
        if constexpr (NM == kNu3Array) {
            const __amdgpu_buffer_rsrc_t rn = prsrc(a.nu_arr, z + 1 < z1 ? z + 1 : -1);
#pragma unroll
            for (int r = 0; r < R; ++r) Nn[r] = pldv<float, VEC>(rn, ro[r + 1]);
        }
        [[maybe_unused]] Cells<float, VEC> Tn[R];
        if constexpr (BUOY) {
            // no plane past the chunk: z1 + 1 is outside the window, periodic or not
            const __amdgpu_buffer_rsrc_t rtn = prsrc(a.T, z + 1 < z1 ? z + 1 : z1 + 1);
#pragma unroll
            for (int r = 0; r < R; ++r) Tn[r] = pldv<float, VEC>(rtn, ro[r + 1]);
        }
        // two planes ahead
        const Plane<VEC, R> Un = load_plane(a.u, z + 2), Vn = load_plane(a.v, z + 2), Wn = load_plane(a.w, z + 2);
        const bool zin = ZPER || (z >= 1 && z <= nz - 2);  // wave-uniform
        const size_t pofs = (size_t)z * plane;
        const __amdgpu_buffer_rsrc_t rus = __builtin_amdgcn_make_buffer_rsrc(a.us + pofs, 0, pbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rvs = __builtin_amdgcn_make_buffer_rsrc(a.vs + pofs, 0, pbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rws = __builtin_amdgcn_make_buffer_rsrc(a.ws + pofs, 0, pbytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rt =
            __builtin_amdgcn_make_buffer_rsrc(a.tau ? a.tau + pofs : a.us, 0, a.tau ? pbytes : 0, 0x00020000);
        [[maybe_unused]] __amdgpu_buffer_rsrc_t rnt = rt;
        if constexpr (NM == kNu3Les)
            rnt = __builtin_amdgcn_make_buffer_rsrc(a.nut ? a.nut + pofs : a.us, 0, a.nut ? pbytes : 0, 0x00020000);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = j0 + r;
            // the six faces keep f (tau, nu_t: 0)
            Cells<float, VEC> uo = Uc.row[r + 1], vo = Vc.row[r + 1], wo = Wc.row[r + 1], to = {};
            [[maybe_unused]] Cells<float, VEC> no = {};
            if (zin && j >= 1 && j <= ny - 2) {  // wave-uniform
                const float *uc = Uc.row[r + 1].x, *vc = Vc.row[r + 1].x, *wc = Wc.row[r + 1].x;
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    Nb7 fu, fv, fw;
                    fu.C = uc[c];
                    fv.C = vc[c];
                    fw.C = wc[c];
                    fu.E = c < VEC - 1 ? uc[c + 1] : dpp_from_upper_old(Uc.halo[r], uc[0]);
                    fu.W = c > 0 ? uc[c - 1] : dpp_from_lower_old(Uc.halo[r], uc[VEC - 1]);
                    fv.E = c < VEC - 1 ? vc[c + 1] : dpp_from_upper_old(Vc.halo[r], vc[0]);
                    fv.W = c > 0 ? vc[c - 1] : dpp_from_lower_old(Vc.halo[r], vc[VEC - 1]);
                    fw.E = c < VEC - 1 ? wc[c + 1] : dpp_from_upper_old(Wc.halo[r], wc[0]);
                    fw.W = c > 0 ? wc[c - 1] : dpp_from_lower_old(Wc.halo[r], wc[VEC - 1]);
                    fu.N = Uc.row[r + 2].x[c];
                    fu.S = Uc.row[r].x[c];
                    fv.N = Vc.row[r + 2].x[c];
                    fv.S = Vc.row[r].x[c];
                    fw.N = Wc.row[r + 2].x[c];
                    fw.S = Wc.row[r].x[c];
                    fu.U = Up.row[r + 1].x[c];
                    fu.D = Um[r].x[c];
                    fv.U = Vp.row[r + 1].x[c];
                    fv.D = Vm[r].x[c];
                    fw.U = Wp.row[r + 1].x[c];
                    fw.D = Wm[r].x[c];
                    const bool in = x0 + c >= 1 && x0 + c <= nx - 2;
                    float ne = nu;  // the cell's nu_eff
                    if constexpr (NM == kNu3Array) ne = Nc[r].x[c];
                    if constexpr (NM == kNu3Les) {
                        const float nt = smag3_nut(fu, fv, fw, a.c2, a.k);
                        ne = (nu + nt) + a.art;
                        no.x[c] = in ? nt : 0.0f;
                    }
                    float t = 0.0f;
                    if constexpr (SUPG) t = pred3_tau(uc[c], vc[c], wc[c], ne, dt, a.k);
                    float nu_ = pred3_cell<SUPG>(uc[c], vc[c], wc[c], fu, t, ne, dt, a.k);
                    float nv_ = pred3_cell<SUPG>(uc[c], vc[c], wc[c], fv, t, ne, dt, a.k);
                    float nw_ = pred3_cell<SUPG>(uc[c], vc[c], wc[c], fw, t, ne, dt, a.k);
                    if constexpr (BUOY) {
                        const float th = Tc[r].x[c] - a.t_ref;
                        nu_ = nu_ + dt * (a.bx * th);
                        nv_ = nv_ + dt * (a.by * th);
                        nw_ = nw_ + dt * (a.bz * th);
                    }
                    uo.x[c] = in ? nu_ : uc[c];
                    vo.x[c] = in ? nv_ : vc[c];
                    wo.x[c] = in ? nw_ : wc[c];
                    to.x[c] = in ? t : 0.0f;
                }
            }
            const uint32_t o = ro[r + 1];
            pstv<float, VEC>(uo, rus, o);
            pstv<float, VEC>(vo, rvs, o);
            pstv<float, VEC>(wo, rws, o);
            if (a.tau) pstv<float, VEC>(to, rt, o);  // zeros without SUPG
            if constexpr (NM == kNu3Les)
                if (a.nut) pstv<float, VEC>(no, rnt, o);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            Um[r] = Uc.row[r + 1];
            Vm[r] = Vc.row[r + 1];
            Wm[r] = Wc.row[r + 1];
        }
        Uc = Up;
        Vc = Vp;
        Wc = Wp;
        Up = Un;
        Vp = Vn;
        Wp = Wn;
        if constexpr (NM == kNu3Array) {
#pragma unroll
            for (int r = 0; r < R; ++r) Nc[r] = Nn[r];
        }
        if constexpr (BUOY) {
#pragma unroll
            for (int r = 0; r < R; ++r) Tc[r] = Tn[r];
        }
    }
}

template <int VEC, int R, int NM, bool ZPER = false, bool BUOY = false>
inline const void *pred_planes_kernel_nm(bool supg) {
    return supg ? (const void *)k_predictor3d_planes<VEC, R, true, NM, ZPER, BUOY>
                : (const void *)k_predictor3d_planes<VEC, R, false, NM, ZPER, BUOY>;
}
template <int VEC, int R, bool BUOY = false>
inline const void *pred_planes_kernel(bool supg, int nm, bool zper) {
    if (zper)  // scalar and LES only (the caller has no periodic array mode)
        return nm == kNu3Les ? pred_planes_kernel_nm<VEC, R, kNu3Les, true, BUOY>(supg)
                             : pred_planes_kernel_nm<VEC, R, kNu3Scalar, true, BUOY>(supg);
    if constexpr (!BUOY)  // no buoyant array mode either
        if (nm == kNu3Array) return pred_planes_kernel_nm<VEC, R, kNu3Array>(supg);
    if (nm == kNu3Les) return pred_planes_kernel_nm<VEC, R, kNu3Les, false, BUOY>(supg);
    return pred_planes_kernel_nm<VEC, R, kNu3Scalar, false, BUOY>(supg);
}

// Plane-march launch: cells per lane vec (1, 2, 4), rows per wave rows (1, 2),
// planes per chunk zchunk (0: auto), zper: periodic z (not with kNu3Array);
// a.nseg / a.ntile / a.zchunk are filled here.  The caller has checked shape
// (a plane below 2^31 bytes, nx % vec == 0) and alignment.  BUOY: the buoyant
// instantiations (a.T, a.bx .. a.t_ref set; not with kNu3Array).
template <bool BUOY = false>
inline hipError_t pred_planes_launch(Pred3Args a, bool supg, int nm, int vec, int rows, int zchunk, hipStream_t s,
                                     bool zper = false) {
    const void *f;
    if (rows == 1)
        f = vec == 4   ? pred_planes_kernel<4, 1, BUOY>(supg, nm, zper)
            : vec == 2 ? pred_planes_kernel<2, 1, BUOY>(supg, nm, zper)
                       : pred_planes_kernel<1, 1, BUOY>(supg, nm, zper);
    else
        f = vec == 4   ? pred_planes_kernel<4, 2, BUOY>(supg, nm, zper)
            : vec == 2 ? pred_planes_kernel<2, 2, BUOY>(supg, nm, zper)
                       : pred_planes_kernel<1, 2, BUOY>(supg, nm, zper);
    a.nseg = ceil_div(a.nx, 64 * vec);
    a.ntile = ceil_div(a.ny, 4 * rows);
    // planes per chunk: each chunk re-reads 2 planes, so long chunks, but at
    // least ~2048 workgroups where the grid has them: 8 .. 32 planes
    a.zchunk = zchunk;
    if (a.zchunk <= 0) {
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
