// fields2d.hip -- predictor (advection-diffusion), divergence, projection,
// step epilogue and diagnostic reductions of the v5 cylinder solver's
// time_step(), v5.py:375-441, for gfx950, on float32 fields
// (memory_efficient=True, the reference's configuration).
//
// The one-thread-per-cell kernels and their launchers are the float
// instantiations of fields2d_cells.hpp.  Arithmetic follows the reference as
// it executes in NumPy-scalar form: every Python-float constant is rounded to
// float32 where it meets float32 data (NEP 50), operations run in float32 in
// the source order, nothing is fused (-ffp-contract=off).  |V| = (u**2 +
// v**2) ** 0.5 goes through the device copy of glibc's powf (libm_powf.hpp),
// as NumPy's float32 scalar `**` does in the reference, so the predictor is
// bit-exact too.
//
// This file adds what only the float32 step has: clean_divergence_fast's phi
// sweep on a skewed copy of phi and div, and the predictor's tuning entry
// points.
#include <atomic>
#include <map>
#include <mutex>

#include "fields2d_cells.hpp"

namespace cfd {

// ------------------------------------------------------------ epilogue
// clean_divergence_fast's phi sweep (v5.py:250-253) in the serial
// lexicographic order; k_lex_gs_sweep (fields2d_cells.hpp) says why walking
// the anti-diagonals reproduces the serial loop exactly.
//
// The sweep on a SKEWED copy of phi and div (r05, the default): the r02-r04
// staged kernels kept phi row-major, so the diagonal a wave touches per step
// (lane l: row r0 + l, column d - l) is 64 cache lines, and a CU's vector
// memory path moves about one line per clock -- measured 90-100 us per
// 600-column sweep, several times the ~47-cycle dependent chain per step
// (scripts/chain_probe.hip).  clean_divergence owns its phi and div (the
// workspace), so it stores them diagonal-major instead:
//   rows in blocks of 64 (block m: rows 1 + 64 m + l, l < 64); within a
//   block, diagonal d = j + l in groups of four:
//     (m, d, l) -> ((m DG + d / 4) 64 + l) 4 + d % 4,   DG = ceil((nx + 63) / 4)
// so a wave's four consecutive steps of one field -- lane l's slots d .. d + 3
// -- are one coalesced 1-KB dwordx4.  The grid-wide kernels pay the scatter
// instead (k_divergence_skew writes div there, k_sub_gradient_skew reads phi
// there), spread over every CU.
// Per wave (one 64-row block, one lane per row, up to 4 waves per band), at
// step d lane l updates column j = d - l:
//  * E (old phi of its row at j + 1) is slot d + 1 of its own row;
//  * N (old phi of row r + 1 at j) is lane l + 1's E of the same step (DPP);
//    lane 63's is the next block's lane 0 at slot d - 63;
//  * S (new phi of row r - 1 at j) is lane l - 1's previous result (DPP);
//    lane 0's is the wave above's last lane, published per 16 steps into an
//    LDS row with a counter, or for a band's first wave the block above's
//    lane 63 at slot d + 63 (final: the band before);
//  * the operands stream kSkewRing groups of four steps ahead in registers
//    (the two rows from other blocks by lanes 63 and 0 alone); results leave
//    four steps at a time (0 at the zero side columns and the padding).
// Same arithmetic and order as the serial loop: bit-identical.
constexpr size_t kLexLdsMax = 160 * 1024;  // LDS a sweep workgroup may take
constexpr int kSkewWaves = 4;  // waves per band: at one wave per SIMD the chain, not the memory path, sets the pace
constexpr int kSkewRing = 8;   // groups of 4 steps in flight per wave (and per loop iteration)
constexpr int kSkewMcBlocks = 128;        // k_lex_gs_skew_mc: blocks (workgroups) at most
constexpr size_t kSkewMcLds = 64 * 1024;  // k_lex_gs_skew_mc: LDS asked for (unused; two per CU at most)
__host__ __device__ inline int lex_skew_blocks(int ny) { return (ny - 2 + 63) >> 6; }
__host__ __device__ inline int lex_skew_groups(int nx) { return (nx + 63 + 3) >> 2; }
size_t lex_skew_floats(int ny, int nx) { return (size_t)lex_skew_blocks(ny) * (size_t)lex_skew_groups(nx) * 256; }
// the per-block progress words of k_lex_gs_skew_mc, after div and the two phi
size_t lex_skew_prog_offset(int ny, int nx) { return (3 * sizeof(float) * lex_skew_floats(ny, nx) + 255) & ~(size_t)255; }
// floats per wave row of k_lex_gs_skew's LDS: column c at c + 64 for
// c = -63 .. nx + 76, 16 B aligned
constexpr int lex_skew_rsl(int nx) { return (nx + 160 + 3) & ~3; }
size_t lex_skew_lds_bytes(int nw, int nx) { return (size_t)nw * lex_skew_rsl(nx) * sizeof(float); }
__device__ inline size_t skew_at(int i, int j, int dg) {  // interior row i >= 1, column j >= 0
    const int m = (i - 1) >> 6, l = (i - 1) & 63, d = j + l;
    return (((size_t)m * dg + (d >> 2)) * 64 + l) * 4 + (d & 3);
}

// compute_divergence_fast (v5.py:178-187) into the skewed layout: interior
// rows, every column (0 at the side columns, as k_divergence).  With zphi the
// grid has one more row, ny - 1, and zphi gets zeros on row ny - 1 when that
// row is a lane of the last block: the first sweep leaves the rows past ny - 2
// unwritten, and the next sweep reads that one as the last row's N.
__global__ __launch_bounds__(256) void k_divergence_skew(const float *__restrict__ u, const float *__restrict__ v,
                                                         float *__restrict__ div_s, float *__restrict__ zphi, int ny,
                                                         int nx, float cx, float cy) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y + 1;
    if (j >= nx) return;
    const int dg = lex_skew_groups(nx);
    if (i == ny - 1) {  // zphi only
        if (((ny - 2) & 63) != 0) zphi[skew_at(i, j, dg)] = 0.0f;
        return;
    }
    const size_t c = (size_t)i * nx + j;
    float d = 0.0f;
    if (j >= 1 && j <= nx - 2) d = (u[c + 1] - u[c - 1]) * cx + (v[c + nx] - v[c - nx]) * cy;
    div_s[skew_at(i, j, dg)] = d;
}

// u -= dphi/dx, v -= dphi/dy (v5.py:255-256) with phi in the skewed layout
// (rows 0 and ny - 1 are the zero boundary).
__device__ inline float skew_phi(const float *phi_s, int i, int j, int ny, int dg) {
    return i >= 1 && i <= ny - 2 ? phi_s[skew_at(i, j, dg)] : 0.0f;
}
__global__ void k_sub_gradient_skew(const float *__restrict__ phi_s, float *__restrict__ u, float *__restrict__ v,
                                    int ny, int nx, float cx, float cy) {
    CFD_2D_INDEX
    if (!interior(i, j, ny, nx)) return;
    const int dg = lex_skew_groups(nx);
    const float a = (skew_phi(phi_s, i, j + 1, ny, dg) - skew_phi(phi_s, i, j - 1, ny, dg)) * cx;
    const float b = (skew_phi(phi_s, i + 1, j, ny, dg) - skew_phi(phi_s, i - 1, j, ny, dg)) * cy;
    u[c] = u[c] - a;
    v[c] = v[c] - b;
}

// clean_divergence's second iteration without materialising the first one's
// u, v (iterations == 2, the reference's call, v5.py:430): div of
// u1 = u - dphi1/dx, v1 = v - dphi1/dy, each neighbour's u1 / v1 re-formed with
// k_sub_gradient_skew's operations (the boundary ring keeps u, v), then
// k_divergence's -- the same bits as the three launches.
__global__ __launch_bounds__(256) void k_divergence2_skew(const float *__restrict__ u, const float *__restrict__ v,
                                                          const float *__restrict__ phi1, float *__restrict__ div_s,
                                                          int ny, int nx, float cx, float cy) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y + 1;
    if (j >= nx) return;
    const int dg = lex_skew_groups(nx);
    float d = 0.0f;
    if (j >= 1 && j <= nx - 2) {
        auto u1 = [&](int jj) {
            const float u0 = u[(size_t)i * nx + jj];
            if (jj < 1 || jj > nx - 2) return u0;
            const float a = (skew_phi(phi1, i, jj + 1, ny, dg) - skew_phi(phi1, i, jj - 1, ny, dg)) * cx;
            return u0 - a;
        };
        auto v1 = [&](int ii) {
            const float v0 = v[(size_t)ii * nx + j];
            if (ii < 1 || ii > ny - 2) return v0;
            const float b = (skew_phi(phi1, ii + 1, j, ny, dg) - skew_phi(phi1, ii - 1, j, ny, dg)) * cy;
            return v0 - b;
        };
        d = (u1(j + 1) - u1(j - 1)) * cx + (v1(i + 1) - v1(i - 1)) * cy;
    }
    div_s[skew_at(i, j, dg)] = d;
}

// both iterations' u -= dphi/dx, v -= dphi/dy in one pass: (u - a1) - a2, the
// two in-place subtractions' bits
__global__ void k_sub_gradient2_skew(const float *__restrict__ phi1, const float *__restrict__ phi2,
                                     float *__restrict__ u, float *__restrict__ v, int ny, int nx, float cx, float cy) {
    CFD_2D_INDEX
    if (!interior(i, j, ny, nx)) return;
    const int dg = lex_skew_groups(nx);
    const float a1 = (skew_phi(phi1, i, j + 1, ny, dg) - skew_phi(phi1, i, j - 1, ny, dg)) * cx;
    const float b1 = (skew_phi(phi1, i + 1, j, ny, dg) - skew_phi(phi1, i - 1, j, ny, dg)) * cy;
    const float a2 = (skew_phi(phi2, i, j + 1, ny, dg) - skew_phi(phi2, i, j - 1, ny, dg)) * cx;
    const float b2 = (skew_phi(phi2, i + 1, j, ny, dg) - skew_phi(phi2, i - 1, j, ny, dg)) * cy;
    u[c] = (u[c] - a1) - a2;
    v[c] = (v[c] - b1) - b2;
}

struct SkewArgs {
    float *phi_base;  // the skewed phi buffers (phi_bytes in all)
    const float *div_s;
    unsigned long long *prog;  // MC: per block {epoch, groups stored and complete}
    int *fail;                 // MC: the device's persistent-failure counter
    unsigned long long poll_ticks;
    int phi_bytes, old_off, new_off;  // old_off kOob: all zeros (the first sweep)
    int ny, nx;
    unsigned epoch;
    float cx, cy, cd;
};

// One wave's sweep of block m.  !MC: up to 4 waves per band share a workgroup
// (one CU), lane 0's row above from the wave above through an LDS row, a
// band's first wave (FIRST) from memory.  MC (r05): one wave per workgroup,
// every block on its own CU, each wave FIRST: lane 0's row above is block
// m - 1's lane 63 in the new buffer, read with sc1 loads once block m - 1 has
// published (sc1, per 16 steps) that those groups are stored and complete;
// the progress word is polled two chunks ahead, so the poll's wait is the
// ring's own.
template <bool MC>
__device__ inline void lex_skew_wave(const SkewArgs &sa, int m, int wv, int nw, int lane, float *lex_rows,
                                     int *flags) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    constexpr int R = kSkewRing;
    constexpr int XA = MC ? 16 : 0;  // sc1 on the cross-block loads and the stores
    const int old_off = sa.old_off, new_off = sa.new_off;
    const float cx = sa.cx, cy = sa.cy, cd = sa.cd;
    const int RSL = lex_skew_rsl(sa.nx);
    const int imax = sa.ny - 2, jmax = sa.nx - 2;
    const int nb = lex_skew_blocks(sa.ny), DG = lex_skew_groups(sa.nx);
    const int bytes = nb * DG * 1024;
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(sa.phi_base, 0, sa.phi_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rd =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(sa.div_s), 0, bytes, 0x00020000);
    // steps d = 0 .. 4 DG - 1, 16 per chunk: every slot of the block is stored
    // (lane 63's last interior column is at d = nx + 61, its zero side column
    // at nx + 62, and the padding up to 4 DG - 1 is written too)
    const int nq = (DG + 3) >> 2;
    const int nc = (nq + R / 4 - 1) / (R / 4);  // loop iterations of 4 R steps
    const bool rowok = 1 + 64 * m + lane <= imax;
    // byte offsets of group 0 (group G at + 1024 G): own slots (div; old
    // phi; new phi); lane 63: the next block's lane 0, group G - 16, old;
    // lane 0 of a band's first wave: the block above's lane 63, group
    // G + 15, new.  (kOob + an offset stays past the buffer.)
    const int oD = (m * DG * 64 + lane) * 16;
    const int oS = old_off + oD;
    const int oX = lane == 63 ? (m + 1 < nb ? old_off + ((m + 1) * DG - 16) * 1024 : (int)kOob)
                   : lane == 0 && (MC || wv == 0) && m > 0 ? new_off + (((m - 1) * DG + 15) * 64 + 63) * 16
                                                    : (int)kOob;
    const int oW = rowok ? new_off + oD : (int)kOob;
    float *mine = MC ? nullptr : lex_rows + (size_t)wv * RSL + 64;
    const float *above = MC ? nullptr : lex_rows + (size_t)(wv > 0 ? wv - 1 : 0) * RSL + 64;
    // MC: block m - 1's progress (groups stored and complete), the two polls
    // in flight (issued two and one chunks back) and what is known so far
    unsigned long long poll_a = 0, poll_b = 0;
    int known = 0;
    // the in-flight polls must stay vector registers: a value the compiler
    // sees as uniform is moved to scalar registers right after its load,
    // which waits for it (and, memory operations completing in order, for
    // the whole prefetch ring) -- an opaque lane-dependent zero in the
    // address keeps it per lane until it is used, two chunks later
    int vz = 0;
    __asm__ volatile("" : "+v"(vz));
    unsigned long long *const prog_up = MC && m > 0 ? sa.prog + (m - 1) + vz : nullptr;
    auto progress_of = [&](unsigned long long v) {
        return (unsigned)(v >> 32) == sa.epoch ? (int)(unsigned)(v & 0x7fffffffull) : 0;
    };
    // a software pipeline of R groups: iteration c computes groups R c ..
    // R c + R - 1 and loads groups R (c + 1) + g into the slots it frees;
    // it starts at c = -1, whose steps only load (no lane is at a column
    // >= 1 there: nothing is stored or kept), so the loop has one shape
    // and the compiler's wait counts are the steady-state ones
    f4v P[R], D[R], X[R];
    float w, vprev;  // w: phi(i, j - 1)
    // !FIRST: the row above for the next chunk, read one chunk ahead, and the
    // wave above's count read just before it
    float S0n[16];
    int s0_flag = 0;
    auto s0_read = [&](int q) {
        __asm__ volatile("" ::: "memory");  // after the count read, in issue order
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float4 a4 = *reinterpret_cast<const float4 *>(above + 16 * q + 4 * p);
            S0n[4 * p] = a4.x;
            S0n[4 * p + 1] = a4.y;
            S0n[4 * p + 2] = a4.z;
            S0n[4 * p + 3] = a4.w;
        }
    };
    // One 16-step chunk (ring slots 4 H .. 4 H + 3).  The step is issue-
    // bound (a wave64 VALU op takes 4 cycles: ~13 per step were ~55 cycles
    // against the ~47-cycle dependent chain), so the chunk is specialised:
    // FULL chunks -- every lane at a column 1 .. nx - 2 in all 16 steps,
    // most of a sweep -- skip the per-step column test and the selects;
    // FIRST (a band's first wave) takes lane 0's row above from X, the
    // others from the LDS row, without a per-step select.
    auto chunk = [&](auto Hc, auto FULLc, auto FIRSTc, int qc) {
        constexpr int H = decltype(Hc)::value;
        constexpr bool FULL = decltype(FULLc)::value, FIRST = decltype(FIRSTc)::value;
        float S0[16];
        if constexpr (!FIRST) {
            if (qc >= 0) {
                // wave w - 1's last lane must have published chunks 0 .. qc + 4
                // (its column 16 qc + 15 comes at its step 16 qc + 78).  The
                // count and the row were read one chunk ago (s0_prefetch);
                // only when that count fell short are they read again here
                const int need = qc + 5 < nq ? qc + 5 : nq;
                if (!(s0_flag >= need)) {
                    while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&flags[wv - 1], __ATOMIC_RELAXED,
                                                                            __HIP_MEMORY_SCOPE_WORKGROUP)) < need)
                        __builtin_amdgcn_s_sleep(1);
                    s0_read(qc);
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) S0[k] = S0n[k];
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) S0[k] = 0.f;
            }
            // the next chunk's count and row, in flight during this chunk: the
            // wait for them no longer stalls a chunk (two LDS round trips a
            // chunk made the waves that read them ~25 % slower per step).
            // LDS operations of a wave run in issue order, and the writer
            // stores the row before the count, so a row read issued after a
            // count read that saw the writer's count holds the row
            if (qc + 1 >= 0 && qc + 1 < nq) {
                s0_flag = __hip_atomic_load(&flags[wv - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                s0_read(qc + 1);
            }
        }
        if constexpr (MC) {
            if (m > 0) {
                // this chunk's refills read block m - 1's groups up to
                // 4 qc + 3 + R + 16: they must be stored and complete
                const unsigned long long v = poll_a;
                poll_a = poll_b;
                poll_b = __hip_atomic_load(prog_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int pv = progress_of(v);
                known = pv > known ? pv : known;
                const int need = 4 * qc + R + 20;
                if (known < need) {  // wait (draining) until two chunks past the need
                    const unsigned long long t0 = wall_clock64();
                    while (true) {
                        const int p2 = progress_of(
                            __hip_atomic_load(sa.prog + (m - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                        known = p2 > known ? p2 : known;
                        if (known >= need + 8 || known == 0x7fffffff) break;
                        if (wall_clock64() - t0 > sa.poll_ticks) {  // fail loudly: counted, results garbage
                            if (lane == 0 && sa.fail) atomicAdd(sa.fail, 1);
                            known = 0x7fffffff;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                }
            }
        }
        // this chunk's group 0 at + sof; the refills R groups later
        const int sof = __builtin_amdgcn_readfirstlane(qc * 4 * 1024);
        float out[16];
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const int g = 4 * H + gg;  // ring slot
            const f4v p0 = P[g], p1 = P[(g + 1) % R], x0 = X[g], x1 = X[(g + 1) % R], d4 = D[g];
            f4v o4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float e = k < 3 ? p0[k + 1] : p1[0];   // slot d + 1
                const float xn = k < 3 ? x0[k + 1] : x1[0];  // lane 63: slot d - 63
                float s0;
                if constexpr (FIRST)
                    s0 = k == 0 ? x0[3] : x1[k - 1];  // lane 0: slot d + 63
                else
                    s0 = S0[4 * gg + k];
                const float n = __int_as_float(__builtin_amdgcn_update_dpp(
                    __float_as_int(xn), __float_as_int(e), 0x130, 0xf, 0xf, false));  // wave_shl:1
                const float S = __int_as_float(__builtin_amdgcn_update_dpp(
                    __float_as_int(s0), __float_as_int(vprev), 0x138, 0xf, 0xf, false));  // wave_shr:1
                const float a = cx * (e + w);
                const float bb = cy * (n + S);
                const float v = ((a + bb) - d4[k]) * cd;
                if constexpr (FULL) {
                    w = v;
                    o4[k] = v;
                } else {
                    const int j = 16 * qc + 4 * gg + k - lane;  // step d = 16 qc + 4 gg + k
                    const bool act = (uint32_t)(j - 1) < (uint32_t)jmax;
                    w = act ? v : w;
                    o4[k] = act ? v : 0.f;  // the side columns and the padding stay 0
                }
                vprev = v;
                out[4 * gg + k] = v;
            }
            // (groups past the block's DG belong to the next block: the
            // loop's last iteration runs up to 8 groups past the end)
            const bool gok = FULL || (qc >= 0 && 4 * qc + gg < DG);
            __builtin_amdgcn_raw_buffer_store_b128(o4, rp, gok ? oW + 1024 * gg : (int)kOob, sof, XA);
            // group G + R's operands into the slot just freed (after its
            // last use: a load issued before it would need a second
            // register and a copy that waits for the load).  Slot g is
            // also read by group G - 1 (done), slot g + 1 by this group
            // (refilled next).
            P[g] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rp, oS + 1024 * gg,
                                                                                  sof + R * 1024, 0));
            D[g] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rd, oD + 1024 * gg,
                                                                                  sof + R * 1024, 0));
            // (all lanes load X though only lane 63 -- and lane 0 of a
            // band's first wave -- reads it: exec-masking the load to
            // those lanes measured 8-11 % slower, r05)
            X[g] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rp, oX + 1024 * gg,
                                                                                  sof + R * 1024, XA));
            // keep the prefetch where it is: the scheduler would sink it
            // next to its use, R groups later, exposing the latency
            __builtin_amdgcn_sched_barrier(0);
        }
        if (wv + 1 < nw && qc >= 0 && lane == 63) {
            // publish the last lane's 16 results (columns 16 qc - 63 + k)
#pragma unroll
            for (int k = 0; k < 16; ++k) mine[16 * qc - 63 + k] = out[k];
            // the row before the count (LDS completes in order; this keeps
            // the compiler from sinking the row writes past the flag)
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __hip_atomic_store(&flags[wv], qc + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if constexpr (MC) {
            // groups stored and complete: the operands of group 4 qc + 3, just
            // consumed (the compiler's wait came before their first use), were
            // loaded after the store of group 4 qc + 3 - R, and memory
            // operations complete in order
            const int cnt = 4 * qc + 4 - R;
            __asm__ volatile("" ::: "memory");
            if (cnt > 0 && lane == 0)
                __hip_atomic_store(sa.prog + m, ((unsigned long long)sa.epoch << 32) | (unsigned)cnt, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    using T1 = std::true_type;
    using F0 = std::false_type;
    static_assert(R == 8, "two 16-step chunks per iteration");
    using H0 = std::integral_constant<int, 0>;
    using H1 = std::integral_constant<int, 1>;
    // iterations whose two chunks are both FULL: chunk 2 c >= 4 and
    // 16 (2 c + 1) + 15 <= jmax; the loop is split into head, middle and
    // tail loops around them (a per-chunk branch made the register
    // allocator copy the ring at every merge, waiting for its loads)
    const int cf0 = 2, cf1 = (jmax - 31) >= 0 ? (jmax - 31) >> 5 : -1;  // [cf0, cf1]
    const int cm0 = cf1 >= cf0 ? cf0 : nc, cm1 = cf1 >= cf0 ? (cf1 + 1 < nc ? cf1 + 1 : nc) : nc;
    auto run = [&](auto FIRSTc) {
#pragma unroll
        for (int g = 0; g < R; ++g) P[g] = D[g] = X[g] = f4v{0.f, 0.f, 0.f, 0.f};
        w = 0.f;  // column 0 (boundary)
        vprev = 0.f;
        for (int c = -1; c < cm0; ++c) {
            chunk(H0{}, F0{}, FIRSTc, 2 * c);
            chunk(H1{}, F0{}, FIRSTc, 2 * c + 1);
        }
        for (int c = cm0; c < cm1; ++c) {
            chunk(H0{}, T1{}, FIRSTc, 2 * c);
            chunk(H1{}, T1{}, FIRSTc, 2 * c + 1);
        }
        for (int c = cm1; c < nc; ++c) {
            chunk(H0{}, F0{}, FIRSTc, 2 * c);
            chunk(H1{}, F0{}, FIRSTc, 2 * c + 1);
        }
    };
    if constexpr (MC) {
        run(T1{});
        // every group stored and complete (a release: waits for the stores)
        if (lane == 0)
            __hip_atomic_store(sa.prog + m, ((unsigned long long)sa.epoch << 32) | 0x7fffffffull, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_AGENT);
    } else {
        if (wv == 0)
            run(T1{});
        else
            run(F0{});
    }
}

__global__ __launch_bounds__(256) void k_lex_gs_skew(SkewArgs sa) {
    extern __shared__ float lex_rows[];  // [waves][lex_skew_rsl]: wave w's last-lane results, column c at c + 64
    __shared__ int flags[kSkewWaves];    // 16-step chunks wave w's last lane has published
    const int nw = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nb = lex_skew_blocks(sa.ny);
    for (int b0 = 0; b0 < nb; b0 += nw) {
        __threadfence();  // the band before is final and visible (a band's first wave reads its last row)
        __syncthreads();
        if ((int)threadIdx.x < nw) __hip_atomic_store(&flags[threadIdx.x], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        const int m = b0 + wv;
        if (m >= nb) continue;  // wave-uniform
        lex_skew_wave<false>(sa, m, wv, nw, lane, lex_rows, flags);
    }
}

// one block per workgroup (the dynamic LDS the launch asks for keeps at most
// two such workgroups on a CU)
__global__ __launch_bounds__(64) void k_lex_gs_skew_mc(SkewArgs sa) {
    lex_skew_wave<true>(sa, (int)blockIdx.x, 0, 1, (int)threadIdx.x, nullptr, nullptr);
}

// NumPy float32 scalar power (glibc powf, libm_powf.hpp) elementwise: the
// parity hook for the device powf the SUPG tau uses -- at y = 2 and 0.5 the
// exact-path forms it calls (powf_sq / powf_sqrt), else the restatement.
__global__ void k_numpy_powf(const float *__restrict__ x, float y, float *__restrict__ out, size_t n) {
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < n;
         c += (size_t)gridDim.x * blockDim.x)
        out[c] = y == 2.0f ? libm::powf_sq(x[c]) : (y == 0.5f ? libm::powf_sqrt(x[c]) : libm::powf(x[c], y));
}

static thread_local int g_last_pred[3] = {-1, 0, 0};
void set_last_predictor(int path, int tau, int vec) {
    g_last_pred[0] = path;
    g_last_pred[1] = tau;
    g_last_pred[2] = vec;
}
int pred_rows_resident(const void *f) {
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, int> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(dev, f);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int cus = 256, per = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, f, 256, 0) != hipSuccess || per < 1) per = 1;
    return cache[key] = per * cus;
}

}  // namespace cfd

using namespace cfd;

extern "C" {

int cfd_supg_tau2d_f32(const float *u, const float *v, const float *nu_eff, float nu_eff_scalar,
                       float *tau, int ny, int nx, double dx, double dy, float dt, void *stream) {
    return supg_tau2d<float>("supg_tau2d", u, v, nu_eff, nu_eff_scalar, tau, ny, nx, dx, dy, dt, stream);
}

int cfd_convection_supg2d_f32(const float *u, const float *v, const float *phi, const float *tau,
                              float *conv, int ny, int nx, double dx, double dy, void *stream) {
    return convection_supg2d<float>("convection_supg2d", u, v, phi, tau, conv, ny, nx, dx, dy, stream);
}

int cfd_convection_upwind2d_f32(const float *u, const float *v, const float *phi, float *conv,
                                int ny, int nx, double dx, double dy, void *stream) {
    return convection_upwind2d<float>("convection_upwind2d", u, v, phi, conv, ny, nx, dx, dy, stream);
}

int cfd_laplacian2d_f32(const float *phi, const float *nu_eff, float nu_eff_scalar, float *lap,
                        int ny, int nx, double dx, double dy, void *stream) {
    return laplacian2d<float>("laplacian2d", phi, nu_eff, nu_eff_scalar, lap, ny, nx, dx, dy, stream);
}

int cfd_predictor2d_f32(const float *u, const float *v, const float *nu_eff, float nu_eff_scalar,
                        float *u_star, float *v_star, float *tau, int ny, int nx, double dx,
                        double dy, float dt, int use_supg, void *stream) {
    return predictor2d<float>("predictor2d", u, v, nu_eff, nu_eff_scalar, u_star, v_star, tau, ny, nx, dx, dy, dt,
                              use_supg, stream, false, 0.0f, 0.0, nullptr);
}

int cfd_predictor2d_les_f32(const float *u, const float *v, float nu, float art_visc, double cs, float *u_star,
                            float *v_star, float *tau, float *nu_t, int ny, int nx, double dx, double dy, float dt,
                            int use_supg, void *stream) {
    return predictor2d<float>("predictor2d_les", u, v, nullptr, nu, u_star, v_star, tau, ny, nx, dx, dy, dt, use_supg,
                              stream, true, art_visc, cs, nu_t);
}

int cfd_smagorinsky2d_f32(const float *u, const float *v, float *nu_t, int ny, int nx, double dx, double dy,
                          double cs, void *stream) {
    return smagorinsky2d<float>("smagorinsky2d", u, v, nu_t, ny, nx, dx, dy, cs, stream);
}

// 0: auto (row march when the shape allows it), 1: one thread per cell
// (k_predictor), 2: row march; rows per chunk (0: auto); cells per lane
// (0: auto, 1, 2, 4)
int cfd_set_predictor2d_tau_mode(int mode) {
    CFD_REQUIRE(mode == kTauExact || mode == kTauFast, "predictor2d tau mode: 0 (exact) or 1 (fast)");
    tuning().pred_tau = mode;
    return CFD_OK;
}

int cfd_get_predictor2d_tau_mode(void) { return tuning().pred_tau; }

int cfd_get_last_predictor2d_path(int *tau_mode, int *cells_per_lane) {
    if (tau_mode) *tau_mode = g_last_pred[1];
    if (cells_per_lane) *cells_per_lane = g_last_pred[2];
    return g_last_pred[0];
}

int cfd_set_predictor2d_config(int variant, int rows, int cells_per_lane) {
    CFD_REQUIRE(variant >= 0 && variant <= 2 && rows >= 0, "predictor2d config: variant 0..2, rows >= 0");
    CFD_REQUIRE(cells_per_lane == 0 || cells_per_lane == 1 || cells_per_lane == 2 || cells_per_lane == 4,
                "predictor2d config: cells per lane 0 (auto), 1, 2 or 4");
    tuning().pred_variant = variant;
    tuning().pred_rows = rows;
    tuning().pred_vec = cells_per_lane;
    return CFD_OK;
}

int cfd_divergence2d_f32(const float *u, const float *v, float *div, int ny, int nx, double dx,
                         double dy, float *absmax, void *stream) {
    return divergence2d<float>("divergence2d", u, v, div, ny, nx, dx, dy, absmax, stream);
}

int cfd_gradient2d_f32(const float *phi, float *grad_x, float *grad_y, int ny, int nx, double dx,
                       double dy, void *stream) {
    return gradient2d<float>("gradient2d", phi, grad_x, grad_y, ny, nx, dx, dy, stream);
}

int cfd_project2d_f32(const float *phi, const float *u_star, const float *v_star, float *u,
                      float *v, int ny, int nx, double dx, double dy, float dt, float *gradmax,
                      void *stream) {
    return project2d<float>("project2d", phi, u_star, v_star, u, v, ny, nx, dx, dy, dt, gradmax, stream);
}

size_t cfd_clean_divergence_workspace_bytes(int ny, int nx) {
    // scratch fields: phi and div row-major float64 (cfd_clean_divergence2d_f64)
    // or div and two phi in the skewed float32 layout of k_lex_gs_skew,
    // whichever is larger
    const size_t n = (size_t)(ny > 0 ? ny : 0) * (size_t)(nx > 0 ? nx : 0);
    const size_t skew = ny > 2 && nx > 2 ? lex_skew_prog_offset(ny, nx) + 8 * (size_t)lex_skew_blocks(ny) : 0;
    return 2 * sizeof(double) * n > skew ? 2 * sizeof(double) * n : skew;
}

int cfd_clean_divergence2d_f32(float *u, float *v, int ny, int nx, double dx, double dy,
                               int iterations, void *ws, void *stream) {
    CFD_REQUIRE(u && v && ws, "clean_divergence2d: null pointer");
    CFD_SHAPE2D(ny, nx);
    hipStream_t s = as_stream(stream);
    const double dx2_inv = 1.0 / (dx * dx), dy2_inv = 1.0 / (dy * dy);
    const double denom_inv = 1.0 / (2.0 * (dx2_inv + dy2_inv));
    const float cx = (float)(0.5 / dx), cy = (float)(0.5 / dy);
    if (ny > 2 && nx > 2 && 2 * lex_skew_floats(ny, nx) * 4 < ((size_t)1 << 31)) {
        // div and two phi buffers in the skewed layout (k_lex_gs_skew): the
        // first sweep starts from phi = 0 (np.zeros_like, v5.py:242) by
        // reading nothing; at iterations == 2 the second sweep writes the
        // second buffer, so both gradients are subtracted in one pass
        const size_t F = lex_skew_floats(ny, nx);
        float *div_s = reinterpret_cast<float *>(ws);
        float *phi1 = div_s + F, *phi2 = phi1 + F;
        const int pbytes = (int)(2 * F * sizeof(float));
        const size_t ldsmax = kLexLdsMax - 1024;
        static const int wmax = [] {
            const char *e = getenv("CFD_LEX_SKEW_WAVES");  // A/B knob: waves per band (1 .. 4)
            const int v = e ? atoi(e) : kSkewWaves;
            return v >= 1 && v <= kSkewWaves ? v : kSkewWaves;
        }();
        int nw = lex_skew_blocks(ny) < wmax ? lex_skew_blocks(ny) : wmax;
        while (nw > 1 && lex_skew_lds_bytes(nw, nx) > ldsmax) --nw;
        // one wave per band neither publishes nor reads a row through LDS (no
        // wave below it, and a band's first wave takes the row above from
        // memory): no dynamic LDS, whatever nx (short, very wide grids)
        const size_t lds = nw > 1 ? lex_skew_lds_bytes(nw, nx) : 0;
        static bool attr_s = false;
        if (!attr_s) {
            CFD_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lex_gs_skew),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsmax));
            attr_s = true;
        }
        // past one band, one block per workgroup (k_lex_gs_skew_mc) up to
        // kSkewMcBlocks blocks: the bands ran one after another on one CU.
        // Within one band the single workgroup stays: the multi-CU wave is
        // ~10 % slower per step (sc1 stores, the polls) and lags its
        // neighbour by ~160 steps (r05: 600 x 180 87 -> 89 us per call with
        // it, 1026^2 504 -> 403 us)
        const int nbk = lex_skew_blocks(ny);
        static const int mc_on = [] {
            const char *e = getenv("CFD_LEX_SKEW_MC");  // A/B knob: 0 = the banded single-workgroup sweep
            return e ? atoi(e) : 1;
        }();
        const bool mc = mc_on && nbk > kSkewWaves && nbk <= kSkewMcBlocks;
        if (mc) {
            static bool attr_mc = false;
            if (!attr_mc) {
                CFD_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_lex_gs_skew_mc),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSkewMcLds));
                attr_mc = true;
            }
        }
        SkewArgs sa;
        sa.phi_base = phi1;
        sa.div_s = div_s;
        sa.prog = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(ws) + lex_skew_prog_offset(ny, nx));
        sa.fail = mc ? persist_fail_word(s) : nullptr;
        sa.poll_ticks = persist_poll_ticks();
        sa.phi_bytes = pbytes;
        sa.ny = ny;
        sa.nx = nx;
        sa.cx = (float)dx2_inv;
        sa.cy = (float)dy2_inv;
        sa.cd = (float)denom_inv;
        auto sweep = [&](int old_off, int new_off) {
            sa.old_off = old_off;
            sa.new_off = new_off;
            if (mc) {
                static std::atomic<unsigned> epoch{0};
                unsigned e = epoch.fetch_add(1) + 1;
                if (e == 0) e = epoch.fetch_add(1) + 1;
                sa.epoch = e;
                hipLaunchKernelGGL(k_lex_gs_skew_mc, dim3(nbk), dim3(64), kSkewMcLds, s, sa);
            } else {
                hipLaunchKernelGGL(k_lex_gs_skew, dim3(1), dim3(64 * nw), lds, s, sa);
            }
        };
        const dim3 gr(ceil_div(nx, 256), ny - 2);
        if (iterations >= 1) {
            hipLaunchKernelGGL(k_divergence_skew, dim3(gr.x, ny - 1), dim3(256), 0, s, u, v, div_s, phi1, ny, nx, cx,
                               cy);
            sweep((int)kOob, 0);
        }
        if (iterations == 2) {
            hipLaunchKernelGGL(k_divergence2_skew, gr, dim3(256), 0, s, u, v, phi1, div_s, ny, nx, cx, cy);
            sweep(0, (int)(F * sizeof(float)));
            hipLaunchKernelGGL(k_sub_gradient2_skew, grid2d(ny, nx), dim3(256), 0, s, phi1, phi2, u, v, ny, nx, cx,
                               cy);
        } else if (iterations >= 1) {
            hipLaunchKernelGGL(k_sub_gradient_skew, grid2d(ny, nx), dim3(256), 0, s, phi1, u, v, ny, nx, cx, cy);
            for (int it = 1; it < iterations; ++it) {  // in place on phi1
                hipLaunchKernelGGL(k_divergence_skew, gr, dim3(256), 0, s, u, v, div_s, (float *)nullptr, ny, nx, cx,
                                   cy);
                sweep(0, 0);
                hipLaunchKernelGGL(k_sub_gradient_skew, grid2d(ny, nx), dim3(256), 0, s, phi1, u, v, ny, nx, cx, cy);
            }
        }
        CFD_LAUNCH_CHECK();
        return CFD_OK;
    }
    // past the skewed layout's 2^31-byte offsets: the plain wavefront
    return clean_divergence_plain<float>(u, v, ny, nx, dx, dy, iterations, ws, s);
}

int cfd_apply_bc2d_f32(float *u, float *v, const double *y, int ny, int nx, double y_max,
                       double v_inf, int step, void *stream) {
    return apply_bc2d<float>("apply_bc2d", u, v, y, ny, nx, y_max, v_inf, step, stream);
}

int cfd_apply_lid_bc2d_f32(float *u, float *v, int ny, int nx, float u_lid, void *stream) {
    return apply_lid_bc2d<float>("apply_lid_bc2d", u, v, ny, nx, u_lid, stream);
}

int cfd_apply_ibm2d_f32(float *u, float *v, const double *ibm_mask, int n, double force_strength,
                        void *stream) {
    return apply_ibm2d<float>("apply_ibm2d", u, v, ibm_mask, n, force_strength, stream);
}

int cfd_clip_f32(float *a, size_t n, float lo, float hi, void *stream) {
    return clip_field<float>("clip", a, n, lo, hi, stream);
}

int cfd_absmax_f32(const float *a, size_t n, float *out, void *stream) {
    return absmax2<float>("absmax", a, nullptr, n, out, stream);
}

int cfd_absmax2_f32(const float *a, const float *b, size_t n, float *out, void *stream) {
    CFD_REQUIRE(b, "absmax2: null pointer");
    return absmax2<float>("absmax2", a, b, n, out, stream);
}

int cfd_energy_mean2d_f32(const float *u, const float *v, size_t n, double *out, void *stream) {
    return energy_mean2d<float, false>("energy_mean2d", const_cast<float *>(u), const_cast<float *>(v), n, out, 0.0f,
                                       0.0f, stream);
}

int cfd_mean_f32(const float *a, size_t n, double *out, void *stream) {
    return mean_field<float>("mean_f32", a, n, out, stream);
}

int cfd_energy_mean_clip2d_f32(float *u, float *v, size_t n, double *out, float lo, float hi, void *stream) {
    return energy_mean2d<float, true>("energy_mean_clip2d_f32", u, v, n, out, lo, hi, stream);
}

int cfd_apply_bc_ibm2d_f32(float *u, float *v, const double *y, int ny, int nx, double y_max, double v_inf, int step,
                           const double *ibm_mask, double force_strength, void *stream) {
    return apply_bc_ibm2d<float>("apply_bc_ibm2d_f32", u, v, y, ny, nx, y_max, v_inf, step, ibm_mask, force_strength,
                                 stream);
}

int cfd_vorticity_absmax2d_f32(const float *u, const float *v, const uint8_t *mask, int ny, int nx,
                               double dx, double dy, float *out, void *stream) {
    return vorticity2d<float>("vorticity_absmax2d", u, v, mask, nullptr, out, ny, nx, dx, dy, stream);
}

int cfd_vorticity2d_f32(const float *u, const float *v, const uint8_t *mask, float *w, int ny,
                        int nx, double dx, double dy, void *stream) {
    return vorticity2d<float>("vorticity2d", u, v, mask, w, nullptr, ny, nx, dx, dy, stream);
}

int cfd_numpy_powf_f32(const float *x, float y, float *out, size_t n, void *stream) {
    CFD_REQUIRE(x && out, "numpy_powf: null pointer");
    if (n == 0) return CFD_OK;
    hipLaunchKernelGGL(k_numpy_powf, dim3(grid1d(n)), dim3(256), 0, as_stream(stream), x, y, out, n);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_nonfinite_count_f32(const float *a, const float *b, size_t n, int *out, void *stream) {
    return nonfinite_count<float>("nonfinite_count", a, b, n, out, stream);
}

}  // extern "C"

#ifdef CFD_PRED_COUNT
// measurement aid (a -DCFD_PRED_COUNT build only): cells the row march queued
extern "C" unsigned long long cfd_debug_pred_count(int reset) {
    unsigned long long h = 0;
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(&h, HIP_SYMBOL(cfd::g_pred_count), sizeof(h));
    if (reset) {
        const unsigned long long z = 0;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(cfd::g_pred_count), &z, sizeof(z));
    }
    return h;
}
#endif
