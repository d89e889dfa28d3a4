// wfm_fir_geom.h -- the index arithmetic of k_wfm_fir's two FIRs (the audio response, and the low-pass in front of the discriminator)
// as banded-Toeplitz matrix products on the fp32 matrix instruction (v_mfma_f32_16x16x4_f32), and where the kernel's arrays lie in
// LDS.  Plain C++ (no HIP): tests/test_wfm_fir_matrix_host.py compiles it on the host, emulates the blocked products tile by tile and
// holds them to np.convolve.  The audio FIR first:
//
// A workgroup owns kWfmOutB = 1024 consecutive outputs y[o] = sum_p h[p] db[L4 + o - p], p in [0, L4); db[i] is the discriminator
// sample d[s - L4 + i], i < 1024 + L4.  Write o = 256 cg + 16 a + b (column group cg < 4, column a < 16, row b < 16) and substitute
// k = L4 + b - p:
//     Y[b][a] = sum_k A[b][k] B[k][a],   A[b][k] = h[L4 + b - k] (zero outside [0, L4)),   B[k][a] = db[256 cg + 16 a + k],
// k in [0, L4 + 16): every tap of every row exactly once (k = L4 + b - p lies in [b + 1, b + L4]), the rest are the zero corners of
// the band (K / L4 = 1.02 at L4 = 656).  K runs in groups of 16; the matrix instruction takes four k per step, one per lane quarter
// kq = lane >> 4, and group g's step j gives lane (b or a = lane & 15, kq) the index k = 16 g + 4 kq + j -- so a lane's four B
// operands of a group are four CONSECUTIVE db samples at a 16-byte-aligned place (one ds_read_b128; a wave's 64 reads are 1024
// contiguous bytes: no bank conflict, no pad) and its four A operands are four consecutive taps, kept in that order in a device
// table [group][lane][4] (one coalesced 16-byte load per lane and group).  Eight waves: wave w works column group w & 3 over the
// K half w >> 2; a group's four steps start from C = 0 and the fp32 result is folded into per-lane fp64 sums, as the loop this
// replaces folded every 16 taps.
#pragma once

#if defined(__HIPCC__)
#define PG_WFM_GEOM_FN __host__ __device__ inline
#else
#define PG_WFM_GEOM_FN inline
#endif

namespace pg {

constexpr int kWfmMxTile = 16;        // rows and columns of a tile: 256 outputs
constexpr int kWfmMxColGroups = 4;    // tiles per workgroup (kWfmOutB / 256)
constexpr int kWfmMxHalves = 2;       // K halves: kWfmMxColGroups * kWfmMxHalves = 8 waves
constexpr int kWfmMxGroupK = 16;      // k per group: four steps of the 16x16x4 instruction

// groups of 16 k covering K = L4 + 16 (L4 is a multiple of 16)
PG_WFM_GEOM_FN int wfm_mx_groups(int L4) { return L4 / kWfmMxGroupK + 1; }
// K half `half` runs the groups [wfm_mx_half_begin(G, half), wfm_mx_half_begin(G, half + 1))
PG_WFM_GEOM_FN int wfm_mx_half_begin(int G, int half) { return half <= 0 ? 0 : (half == 1 ? (G + 1) / 2 : G); }
// floats in the device table, [G][64][4]
PG_WFM_GEOM_FN int wfm_mx_table_floats(int L4) { return wfm_mx_groups(L4) * 256; }
// the k index lane `lane` feeds in step j of group g
PG_WFM_GEOM_FN int wfm_mx_k(int g, int lane, int j) { return kWfmMxGroupK * g + 4 * (lane >> 4) + j; }
// A operand: the tap index of row b = lane & 15 at that k, or -1 where the band has a zero corner
PG_WFM_GEOM_FN int wfm_mx_tap(int L4, int g, int lane, int j)
{
    const int p = L4 + (lane & 15) - wfm_mx_k(g, lane, j);
    return p >= 0 && p < L4 ? p : -1;
}
// B operand: the db index of column a = lane & 15 of column group cg at that k (j = 0: a multiple of 4)
PG_WFM_GEOM_FN int wfm_mx_db(int cg, int g, int lane, int j) { return 256 * cg + kWfmMxTile * (lane & 15) + wfm_mx_k(g, lane, j); }
// C/D: register r of lane `lane` holds row 4 (lane >> 4) + r of column lane & 15 -> the workgroup's output index
PG_WFM_GEOM_FN int wfm_mx_out(int cg, int lane, int r) { return 256 * cg + kWfmMxTile * (lane & 15) + 4 * (lane >> 4) + r; }

// Where `db` (outb + L4 floats) starts in the kernel's dynamic LDS, in floats.  wfm_fir_lds_bytes (kernels_demod.h) counts NX + NX / 8
// + 1 sample slots and NL + 1 low-passed slots of 8 bytes in front of db; db sits there, moved down by one slot where that sum is odd
// (a 16-byte boundary), so the allocation covers it as it is.  The low-passed planes (wfm_fir_lp_offset) lie directly in front of it
// and the sample planes at the start.
PG_WFM_GEOM_FN int wfm_fir_db_offset(int outb, int L4, int Llp)
{
    const int ND = outb + L4, NL = (ND + 1 + 7) & ~7, NX = NL + Llp - 1;
    const int slots = NX + NX / 8 + 1 + NL + 1;
    return 2 * (slots - (slots & 1));
}

// ---- the low-pass in front (phase 2), the same product with real taps on both components of the complex samples ----
// lp[o] = sum_m hlp[m] x[o + Llp - 1 - m], o < NL.  With o = 256 t + 16 a + b and k = Llp - 1 + b - m: A[b][k] = hlp[Llp - 1 + b - k],
// B[k][a] = x[256 t + 16 a + k], k in [0, Llp + 15) in groups of 16 (at most five: Llp <= 64); the lane maps, wfm_mx_k and wfm_mx_out
// are phase 4's.  Samples and results lie in LDS as two planes each (real parts, imaginary parts): a job is one tile of 256 outputs
// of one plane, wave w runs the jobs w, w + 8, ...; job -> tile job >> 1 of plane job & 1.
constexpr int kWfmLpGroupsMax = 5;
PG_WFM_GEOM_FN int wfm_lp_groups(int Llp) { return (Llp + 15 + kWfmMxGroupK - 1) / kWfmMxGroupK; }
PG_WFM_GEOM_FN int wfm_lp_jobs(int NL) { return 2 * ((NL + 255) / 256); }
// A operand: the tap index at (g, lane, j), or -1
PG_WFM_GEOM_FN int wfm_lp_tap(int Llp, int g, int lane, int j)
{
    const int m = Llp - 1 + (lane & 15) - wfm_mx_k(g, lane, j);
    return m >= 0 && m < Llp ? m : -1;
}
// B operand: the sample index at (tile, g, lane, j) (j = 0: a multiple of 4); the kernel reads zeros from NXp = wfm_lp_plane(NX) on
PG_WFM_GEOM_FN int wfm_lp_x(int t, int g, int lane, int j) { return 256 * t + kWfmMxTile * (lane & 15) + wfm_mx_k(g, lane, j); }
PG_WFM_GEOM_FN int wfm_lp_plane(int NX) { return (NX + 3) & ~3; }  // floats per sample plane: NX and a zero rest up to a multiple of 4
// where the result planes (2 NL floats, 16-byte aligned) start, in floats: directly in front of db
PG_WFM_GEOM_FN int wfm_fir_lp_offset(int outb, int L4, int Llp)
{
    const int NL = (outb + L4 + 1 + 7) & ~7;
    return wfm_fir_db_offset(outb, L4, Llp) - 2 * NL;
}

// the device table from the response h[0 .. L4) (WfmCore::init): table[(g * 64 + lane) * 4 + j]
template <class T>
inline void wfm_mx_fill_taps(const T *h, int L4, float *table)
{
    const int G = wfm_mx_groups(L4);
    for (int g = 0; g < G; g++)
        for (int lane = 0; lane < 64; lane++)
            for (int j = 0; j < 4; j++) {
                const int p = wfm_mx_tap(L4, g, lane, j);
                table[(g * 64 + lane) * 4 + j] = p < 0 ? 0.f : (float)h[p];
            }
}

}  // namespace pg
