// Private to the E-step's units: the argument struct EArgs, the single-pass
// kernel k_estep_mx (J <= 8) with its shape helpers, and the choice of its
// instantiation from the model (estep_dispatch_j), ending in estep_mx_j<J>,
// the one host function that names the kernel.  fasst_em_estep_j<J>.hip
// instantiates estep_mx_j<J> and so holds every k_estep_mx<J, ...>;
// fasst_em_estep.hip calls the eight and instantiates none.
#pragma once
#include "fasst_em.h"
#include "fasst_device.h"

#include <algorithm>

namespace fasst {

// ---------------------------------------------------------------- E-step
struct EArgs {
  const double *cx00, *cx11, *cxr, *cxi;  // [Tp][Fp]
  const double *TW;                       // [J][KP][Tp]
  // tile-packed operand images of k_estep_mx (layouts at the pack kernels)
  const double2 *cxp;                     // [nft][nttp] records of 512: Cx of one 16 x 16 tile
  const double2 *twp;                     // [nttp][J][KP / 8][64]: the tile's TW operand pairs
  const double *Wkf;                      // [J][KP][Fp]
  const double2 *A;                       // [R][2][Fp]
  const double *psd;                      // [Fp]
  double *hatW;                           // [J][Tp][Fp]: rho = hat_W / max(V, eps)
  double *part;                           // [slot][Fp][NACC]
  double *llpart;                         // [slot][nft]
  int F, T, Fp, Tp, KP, R, ntt, tpc, nft;
  int nttp;          // frame tiles of the whole clip (the images' record stride)
  int ybase, tbase;  // this launch's chunks start at partial ybase, frame tile tbase (ntt = end)
  ESched es;         // the partials' layout (k_estep_mx: also its schedule; fasst_esched.h)
  int roff[kMaxJ + 1];
  const int *halt;
};

// Single-pass E-step with the per-bin t-reductions on the matrix cores.
//
// Every statistic of the E-step is a per-bin dot product over frames:
//   cross  Q_j[c]      = sum_t V_j P_c        (P = Cx S, 8 real components)
//   pairs  M_p[c]      = sum_t V_j1 V_j2 N_c  (N = S Cx S - S, 4 components)
// For one bin these are tiny GEMMs, (J x T).(T x 8) and (NP x T).(T x 4).
// v_mfma_f64_4x4x4_4b runs four independent 4x4x4 products per instruction,
// one per block of 16 lanes (lane = 16 X + 4 b + Y: A[m=Y][k=X],
// B[k=X][n=Y], D[m=X][n=Y] of block b; tools/probe_mfma4.hip), so with
// block = bin and k = frame, ONE instruction contracts 4 frames of 4 bins
// for a 4 x 4 block of statistics.  After each frame group, every lane drops
// its point's operands (V, P, N and the pair products V_j1 V_j2) into a
// per-wave LDS slab in the MFMA operand layout, and the wave issues
// 4 bin groups x (2 + ceil(NP/4)) MFMAs.  The accumulators shrink from
// 4 J(J+1)/2 + 8J doubles per lane (72 at J = 4, what forced the round-1
// E-step into two launches) to 4 (2 + ceil(NP/4)) (20 at J = 4), so ONE pass
// streams Cx once, forms V, Sigma_x and its inverse once per point, and keeps
// two waves per SIMD; the 72 FMAs per point leave the VALU for the matrix
// pipe (4x4x4_4b runs at 74.7 TF on this chip, profiles/r1_ubench_fp64.txt).

// Reader-formed pair operands (RP, J >= 4): the slab holds V, P and N only,
// and the reader forms the pair operands V_j1 V_j2 itself.  With the sources
// padded to Q = 4 (J = 4) or 8 (J > 4), lane m of a 4-pair group reads the Q
// rotated values W_e = V_{(m + e) mod Q} of its point, and the pairs are the
// groups (base, d): pair m of a group is (base + m, base + m + d mod Q), its
// operand W_base W_{(base + d) mod Q} -- static register indices.  Q = 8: the
// 36 pairs are {0, 4} x {0..3} plus (0, 4); Q = 4: the 10 pairs are
// (0, 0), (0, 1) and (0, 2) (rows m = 2, 3 of the last repeat rows 0, 1).
// The writer's J (J + 1) / 2 products and their slab stores go (J = 8: 56 ->
// 20 stores per point, J = 4: 26 -> 16), the reader's loads stay or drop
// (J = 8: 14 -> 11 per bin group), and the slab shrinks.  Same-box A/B at
// C3 (J = 4): E-step 0.373 vs 0.390 ms, iteration 1.040 vs 1.068 ms; J = 6 /
// 8 (K = 32): 0.813 / 1.002 ms against 1.083 / 1.663 ms with writer-formed
// pairs.
// VR (J > 4): also the per-source pipelined V tile, one wave per SIMD (the
// register file, not the LDS, bounds it: at two waves the kernel spills
// 500+ bytes per lane to scratch) and the epilogue one bin group at a time.
template <int J>
struct MXShape {
  static constexpr bool VR = J > 4;
  static constexpr bool RP = J >= 4;
  static constexpr int Q = J > 4 ? 8 : 4;       // RP: sources padded to Q
  static constexpr int NP = J * (J + 1) / 2;
  static constexpr int NPG = RP ? (Q == 8 ? 9 : 3) : (NP + 3) / 4;   // pair groups of 4
  static constexpr int NVG = (J + 3) / 4;       // source groups of 4
  static constexpr int SP = NVG, SN = NVG + 2, SV2 = NVG + 3;  // set offsets: P lo/hi, N, VV
  static constexpr int NSET = NVG + 3 + (RP ? 0 : NPG);  // V groups | P lo | P hi | N | VV groups
  static constexpr int GS = NSET * 64 + 1;      // doubles per bin group (+1: bank skew)
  // VST (J > 4): the V sets of all four point rounds are written once per
  // tile, right after the V tile ([round][bin group][NVG sets], VGS each),
  // then P / N per round ([bin group][3 sets], PGS each)
  static constexpr bool VST = VR;
  static constexpr int VGS = NVG * 64 + 1, PGS = 3 * 64 + 1;
  static constexpr int SLAB = VST ? 16 * VGS + 4 * PGS : 4 * GS;   // doubles per wave
};
// RP pair group h: (base, d)
template <int Q>
__host__ __device__ constexpr int rp_base(int h) { return Q == 4 || h == 8 ? 0 : 4 * (h & 1); }
template <int Q>
__host__ __device__ constexpr int rp_d(int h) { return Q == 4 ? h : (h == 8 ? 4 : h >> 1); }
// canonical index (j1 <= j2, j1 major) of the pair lane m of group h
// accumulates, or -1 (a padded source or a repeated pair)
template <int J>
__host__ __device__ constexpr int rp_pair(int h, int m) {
  constexpr int Q = MXShape<J>::Q;
  if (!MXShape<J>::RP) return 4 * h + m < MXShape<J>::NP ? 4 * h + m : -1;
  const int j1 = rp_base<Q>(h) + m, j2 = (rp_base<Q>(h) + m + rp_d<Q>(h)) & (Q - 1);
  if (j1 >= J || j2 >= J || (Q == 4 && rp_d<Q>(h) == 2 && m >= 2)) return -1;
  const int lo = j1 < j2 ? j1 : j2, hi = j1 < j2 ? j2 : j1;
  return lo * J - lo * (lo - 1) / 2 + (hi - lo);
}
// does RP pair group h hold a live pair
template <int J>
__host__ __device__ constexpr bool rp_live(int h) {
  for (int m = 0; m < 4; ++m)
    if (rp_pair<J>(h, m) >= 0) return true;
  return false;
}

// the W tile sits in LDS unless it would push the block past 160 KB (J = 8,
// K = 128); then the V tiles read their W operand from L2
template <int J, int NKS>
__host__ __device__ constexpr bool mx_w_in_lds() {
  return (size_t)(4 + J * 4 * NKS * 16 + 4 * MXShape<J>::SLAB + J * 4 * 16) * sizeof(double) <=
         160 * 1024;
}
template <int J, int NKS>
static constexpr size_t estep_mx_smem() {
  return (size_t)(4 + (mx_w_in_lds<J, NKS>() ? J * 4 * NKS * 16 : 0) + 4 * MXShape<J>::SLAB) *
         sizeof(double);
}

// (the LDS slabs allow two blocks per CU, so the register budget is that of
// two waves per SIMD: amdgpu_waves_per_eu tells the scheduler, which would
// otherwise serialise the operand loads to fit three)
// (more than 4 sources: one block per CU -- the slabs alone pass 80 KB -- so
// one wave per SIMD and the full 512-register file)
// (no-load-store-opt: the compiler otherwise pairs the slab / W-tile reads
// into ds_read2_b64 / ds_read2st64_b64, which take 8 LDS cycles for the 4 of
// two ds_read_b64 -- MI355X_MICROARCH.md §LDS -- and the LDS is this kernel's
// busiest unit)
// raw-buffer forms of the E-step's streaming accesses: wave-uniform
// resource (SGPRs, formed on the scalar unit) + 32-bit per-lane offset, so
// no 64-bit VALU address arithmetic per access (aux 2 = non-temporal)
// (buf_rsrc / buf_ld of fasst_device.h; the store is the E-step's alone)
template <int AUX>
__device__ __forceinline__ void es_st(double v, __amdgpu_buffer_rsrc_t r, unsigned vo, unsigned so) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(buf_u2, v), r, (int)vo, (int)so, AUX);
}

// 16-byte raw-buffer load of an operand image (as buf_ld: wave-uniform
// resource, per-lane byte offset vo, uniform byte offset so)
typedef unsigned buf_u4 __attribute__((ext_vector_type(4)));
typedef double buf_d2 __attribute__((ext_vector_type(2)));
template <int AUX>
__device__ __forceinline__ buf_d2 buf_ld2(__amdgpu_buffer_rsrc_t r, unsigned vo, unsigned so) {
  const buf_u4 x = __builtin_amdgcn_raw_buffer_load_b128(r, (int)vo, (int)so, AUX);
  return __builtin_bit_cast(buf_d2, x);
}

// Does the (J, NKS) instantiation preload every TW operand of a tile in
// pairs of k-steps (the only form that reads the TW image)
template <int J, int NKS>
__host__ __device__ constexpr bool mx_tw_preload() {
  return J <= 4 && J * NKS <= 32 && NKS % 2 == 0;
}

// CXI / TWI: Cx / the preloaded TW operands are read from the tile-packed
// images a.cxp / a.twp (k_cx_image, k_tw_image) instead of the planes: one
// contiguous KB per wave-instruction, 16 bytes per lane, half the loads.
// The values and every arithmetic instruction are those of the plane form.
// (J = 4 at K = 128: the 64 KB W tile leaves one block per CU, so one wave
// per SIMD and the full register file for the pipelined V tile)
template <int J, int NKS, int RKU, bool CXI = false, bool TWI = false>
__global__ __launch_bounds__(256, (J > 4 || (J == 4 && NKS == 32)) ? 1 : 2)
__attribute__((amdgpu_waves_per_eu(1, (J > 4 || (J == 4 && NKS == 32)) ? 1 : 2))) FASST_NO_LDS_PAIRING
void k_estep_mx(const EArgs a) {
  static_assert(!TWI || mx_tw_preload<J, NKS>(), "the TW image serves the preload path only");
  HALT_GUARD(a.halt);
  using S = MXShape<J>;
  constexpr bool VR = S::VR, RP = S::RP;
  constexpr int Q = S::Q;
  constexpr int NP = S::NP, NPG = S::NPG, NVG = S::NVG;
  constexpr int NACC = 4 * NP + 8 * J;
  constexpr int KP = 4 * NKS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // per-source Sigma_x coefficients in a static array: the compiler can see
  // that the slab stores never touch them and reuse each read within a tile
  __shared__ double s_cj[J * 4 * 16];      // [J][4][16]
  constexpr bool WL = mx_w_in_lds<J, NKS>();
  double *s_ll = smem;                     // [4]
  double *s_w = s_ll + 4;                  // [J][KP][16] W tile (if WL)
  double *s_slab = s_w + (WL ? J * KP * 16 : 0);  // [4 waves][SLAB] operand slabs
  double *s_red = s_w;                     // [4][NACC][16 | 4] (epilogue, aliases W + slabs)

  // The block's work: segments, each a run of frame tiles [tb, te) of one
  // 16-bin tile whose statistics go to partial `slot`.  Chunk grid: one
  // segment, (bin tile, chunk) = the XCD-ordered block (x, y).  Balanced
  // schedule (fasst_esched.h): the quad-steps [wu, wend) of the flattened
  // (bin tile, quad-step) list, cut where the bin tile changes; the XCD order
  // gives each XCD a contiguous run of the list.  All of it is wave-uniform.
  const dim3 bi = xcd_block();   // chunk grid: x: 16-bin tile, y: frame chunk
  // (chunk grid: the one segment)
  int btile = bi.x, tb = a.tbase + bi.y * a.tpc, te = min(tb + a.tpc, a.ntt);
  int slot = a.ybase + bi.y;
  int left = 0;   // balanced: quad-steps of the range after this segment
  if (a.es.bal) {
    // the range's first segment: the only divisions, ahead of the segment loop
    // (inside it their loop-invariant parts stayed live across the tile loop)
    const int blk = bi.x, Q = a.es.Q;
    const long long U = (long long)a.es.nbt * Q;
    const int wu = (int)es_lo(blk, U, a.es.nb), wend = (int)es_lo(blk + 1, U, a.es.nb);
    btile = wu / Q;
    const int q0 = wu - btile * Q, nq = min(Q - q0, wend - wu);
    tb = a.tbase + 4 * q0;
    te = min(tb + 4 * nq, a.ntt);
    slot = blk - es_first(btile, Q, a.es.nbt, a.es.nb);
    left = wend - wu - nq;
  }
  // (pinned to SGPRs: the tile loop's bounds and the buffer resources derive from them)
  btile = __builtin_amdgcn_readfirstlane(btile);
  tb = __builtin_amdgcn_readfirstlane(tb);
  te = __builtin_amdgcn_readfirstlane(te);
  slot = __builtin_amdgcn_readfirstlane(slot);
  left = __builtin_amdgcn_readfirstlane(left);
  for (;;) {
  // launder: every per-thread value (the prologue's, the tile loop's and the
  // epilogue's addresses) is formed per segment from this thread index, as in
  // a kernel of one segment: the compiler would otherwise hoist them out of
  // the segment loop and keep them live across the tile loop, ~30 registers
  int tidp = threadIdx.x;
  asm volatile("" : "+v"(tidp));
  const int tid = tidp, lane = tid & 63, wv = tid >> 6;
  const int fl = lane & 15, tq = lane >> 4;
  double *slab = s_slab + wv * S::SLAB;
  const int f0 = btile * 16;
  const int f = f0 + fl;

  if (WL)
    for (int idx = tidp; idx < J * KP * 16; idx += 256) {
      const int ff = idx & 15, jk = idx >> 4;
      s_w[idx] = a.Wkf[(size_t)jk * a.Fp + f0 + ff];
    }
  // operand slots no point writes (sources >= J, pairs >= NP) stay zero
  for (int idx = tidp; idx < 4 * S::SLAB; idx += 256) s_slab[idx] = 0.0;
  if (tidp < 16) {
    const int ff = f0 + tidp;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      double al = 0, be = 0, gr = 0, gi = 0;
      for (int r = a.roff[j]; r < a.roff[j + 1]; ++r) {
        const double2 a0 = a.A[(size_t)(2 * r) * a.Fp + ff];
        const double2 a1 = a.A[(size_t)(2 * r + 1) * a.Fp + ff];
        al += a0.x * a0.x + a0.y * a0.y;
        be += a1.x * a1.x + a1.y * a1.y;
        gr += a0.x * a1.x + a0.y * a1.y;  // Re a0 conj(a1)
        gi += a0.y * a1.x - a0.x * a1.y;  // Im a0 conj(a1)
      }
      s_cj[(j * 4 + 0) * 16 + tidp] = al;
      s_cj[(j * 4 + 1) * 16 + tidp] = be;
      s_cj[(j * 4 + 2) * 16 + tidp] = gr;
      s_cj[(j * 4 + 3) * 16 + tidp] = gi;
    }
  }
  __syncthreads();

  // CJR (J >= 4): the lane's Sigma_x coefficients in registers for the
  // whole kernel (J = 8: 474 -> 240 LDS reads and 243 -> 84 waits per tile,
  // E-step 1.00 -> 0.98 ms; J = 4: 0.372 -> 0.364 ms, same-box A/B)
  constexpr bool CJR = J >= 4;
  constexpr bool NF = J >= 4;
  double cjr[CJR ? J : 1][4];
  if constexpr (CJR)
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) cjr[j][c] = s_cj[(j * 4 + c) * 16 + fl];
  double inv_rk[J];
#pragma unroll
  for (int j = 0; j < J; ++j)
    inv_rk[j] = RKU ? 1.0 / (double)RKU : 1.0 / (double)(a.roff[j + 1] - a.roff[j]);
  const double psd = a.psd[f];
  const bool fvalid = f < a.F;
  // writer side: this lane's point goes to bin group g = fl / 4, block b = fl % 4, X = tq
  double *wr = slab + (fl >> 2) * S::GS + 16 * tq + 4 * (fl & 3);
  // reader side: operands of lane (X, b, Y) sit at [group][set][lane]
  const double *rd = slab + lane;
  auto slab_fence0 = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // RP: W_e = V_{(m + e) mod Q} of the lane's point (m = Y) sits in set
  // ((m + e) mod Q) / 4 at Y' = (m + e) mod 4 of the same (X, b)
  const double *rdq = slab + (lane & ~3);
  constexpr bool VST = S::VST;
  // VST: this lane's V of round i at wrv + i 4 VGS (+ (j >> 2) 64 + (j & 3)),
  // its P / N at wpn; the reader's V of round i, bin group g at
  // rdq + (4 i + g) VGS, P / N at rpn + g PGS
  double *wrv = slab + (fl >> 2) * S::VGS + 16 * tq + 4 * (fl & 3);
  double *wpn = slab + 16 * S::VGS + (fl >> 2) * S::PGS + 16 * tq + 4 * (fl & 3);
  const double *rpn = slab + 16 * S::VGS + lane;
  int vro[Q];
#pragma unroll
  for (int e = 0; e < Q; ++e) {
    const int j = ((lane & 3) + e) & (Q - 1);
    vro[e] = (j >> 2) * 64 + (j & 3);
  }

  double xacc[4][NVG][2], pacc[4][NPG];  // D operands (4x4 blocks per bin group)
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int vg = 0; vg < NVG; ++vg) xacc[g][vg][0] = xacc[g][vg][1] = 0.0;
#pragma unroll
    for (int h = 0; h < NPG; ++h) pacc[g][h] = 0.0;
  }
  double ll = 0.0, lm = 1.0, lev = 0.0, xmin = 1.0;

  // SA: wave-uniform buffer resources (SGPRs, formed on the scalar unit) +
  // 32-bit per-lane byte offsets instead of one 64-bit VALU address
  // computation per access
  constexpr bool SA = true;
  int wvu = wv;
  if constexpr (SA) wvu = __builtin_amdgcn_readfirstlane(wv);
  const unsigned vo_tw = (unsigned)(tq * a.Tp + fl) * 8u;   // TW[j][k = tq + 4s][t0 + fl]
  const unsigned vo_cx = (unsigned)(tq * a.Fp + f) * 8u;    // plane[t0 + tq + 4i][f]
  [[maybe_unused]] const unsigned vo_img = (unsigned)lane * 16u;            // image piece[lane]
  // Cx of frame tile tt (raw-buffer form; the flat form without SA)
  auto load_cx = [&](int tt, double (&c)[4][4]) {
    const int t0 = tt * 16;
    if constexpr (CXI) {
      // the tile's 8 KB record: piece 2 i + h holds (cx00, cx11) (h = 0) or
      // (cxr, cxi) (h = 1) of the lane's point i
      const __amdgpu_buffer_rsrc_t rc =
          buf_rsrc((const double *)(a.cxp + ((size_t)btile * a.nttp + tt) * 512));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const buf_d2 d = buf_ld2<2>(rc, vo_img, (unsigned)(2 * i) * 1024u);
        const buf_d2 o = buf_ld2<2>(rc, vo_img, (unsigned)(2 * i + 1) * 1024u);
        c[0][i] = d.x;
        c[1][i] = d.y;
        c[2][i] = o.x;
        c[3][i] = o.y;
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (SA) {
        const size_t ro = (size_t)t0 * a.Fp;
        const unsigned so = (unsigned)(4 * i * a.Fp) * 8u;
        c[0][i] = buf_ld<2>(buf_rsrc(a.cx00 + ro), vo_cx, so);
        c[1][i] = buf_ld<2>(buf_rsrc(a.cx11 + ro), vo_cx, so);
        c[2][i] = buf_ld<2>(buf_rsrc(a.cxr + ro), vo_cx, so);
        c[3][i] = buf_ld<2>(buf_rsrc(a.cxi + ro), vo_cx, so);
      } else {
        const size_t off = (size_t)(t0 + tq + 4 * i) * a.Fp + f;
        c[0][i] = __builtin_nontemporal_load(a.cx00 + off);
        c[1][i] = __builtin_nontemporal_load(a.cx11 + off);
        c[2][i] = __builtin_nontemporal_load(a.cxr + off);
        c[3][i] = __builtin_nontemporal_load(a.cxi + off);
      }
    }
  };
  // CXE (J > 4): the next tile's Cx loads are issued right after this
  // tile's last point consumed its Cx (in the pipelined point loop), so they
  // land during the last point's MFMAs and the next tile's V tile (J = 6 /
  // 8: 0.790 / 0.961 -> 0.749 / 0.944 ms; at J = 4, two waves per SIMD,
  // 0.361 -> 0.368 ms: not used there)
  constexpr bool CXE = J > 4;
  double cxv[4][4];
  if (CXE && tb + wvu < te) load_cx(tb + wvu, cxv);
  for (int tt = tb + wvu; tt < te; tt += 4) {
    const int t0 = tt * 16;
    int lofs = 0;  // launder: re-read the loop-invariant LDS data per tile
    asm volatile("" : "+v"(lofs));
    // all TW operands in flight before the first MFMA (the scheduler would
    // otherwise pair each load with its MFMA and wait on every one); with more
    // than 32 operands (J > 4 or K > 32 at J = 4) the sources beyond the first
    // 32 operands load next to their own MFMAs
    // (VR: none up front -- the V loop below pipelines them source by source)
    // CP: more operands than that (J <= 4 at K >= 64): the V tiles as one
    // pipeline of 8-MFMA chunks over (source, k), each chunk's TW operands
    // issued two chunks ahead -- the per-source inline loads left each
    // source's load latency exposed (J = 4, K = 128: 2.70 ms).  (The same
    // pipeline for the VR loop with W from L2, J > 4 at K = 128, crashes
    // ROCm 7.2's compiler at distance 2 and spills 0.4-1.8 KB per lane at 1.)
    constexpr bool CP = !VR && J * NKS > 32;
    constexpr int JA = (VR || CP) ? 1 : (J * NKS <= 32) ? J : (32 / NKS > 0 ? 32 / NKS : 1);
    double twv[JA][NKS];
    if constexpr (TWI) {
      // the tile's TW image: piece (j, u) holds the operands of the k-steps
      // s = 2 u (.x) and 2 u + 1 (.y) of source j
      static_assert(JA == J, "every source preloaded");
      const __amdgpu_buffer_rsrc_t rt =
          buf_rsrc((const double *)(a.twp + (size_t)tt * (J * (NKS / 2) * 64)));
#pragma unroll
      for (int j = 0; j < J; ++j)
#pragma unroll
        for (int u = 0; u < NKS / 2; ++u) {
          const buf_d2 h = buf_ld2<0>(rt, vo_img, (unsigned)(j * (NKS / 2) + u) * 1024u);
          twv[j][2 * u] = h.x;
          twv[j][2 * u + 1] = h.y;
        }
    }
#pragma unroll
    for (int j = 0; j < ((CP || TWI) ? 0 : JA); ++j) {
      const double *tw = a.TW + ((size_t)j * KP + tq) * a.Tp + t0 + fl;
#pragma unroll
      for (int s = 0; s < NKS; ++s)
        twv[j][s] = SA ? buf_ld<0>(buf_rsrc(a.TW + t0), vo_tw, (unsigned)((j * KP + 4 * s) * a.Tp) * 8u)
                       : tw[(size_t)(4 * s) * a.Tp];
    }
    if constexpr (!CXE) load_cx(tt, cxv);  // this tile's Cx (in flight with the TW operands)
    __builtin_amdgcn_sched_barrier(0);
    d4 v[J];
    if constexpr (CP) {
      constexpr int CH = 8, CPS = NKS / CH, NCH = J * CPS, PD = 2;   // chunks, prefetch distance
      static_assert(NKS % CH == 0, "k chunks of 8");
      double ta[PD + 1][CH], wa[PD + 1][WL ? 1 : CH];
      auto ld = [&](int u, int sl) {
        const int j = u / CPS, s0 = (u % CPS) * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          const int s = s0 + c;
          ta[sl][c] = buf_ld<0>(buf_rsrc(a.TW + t0), vo_tw, (unsigned)((j * KP + 4 * s) * a.Tp) * 8u);
          if constexpr (!WL)
            wa[sl][c] = a.Wkf[lofs + ((size_t)j * KP + tq + 4 * s) * a.Fp + f];
        }
      };
#pragma unroll
      for (int u = 0; u < PD; ++u) ld(u, u);
#pragma unroll
      for (int u = 0; u < NCH; ++u) {
        if (u + PD < NCH) ld(u + PD, (u + PD) % (PD + 1));
        __builtin_amdgcn_sched_barrier(0);
        const int j = u / CPS, s0 = (u % CPS) * CH, sl = u % (PD + 1);
        if (s0 == 0) v[j] = d4{0.0, 0.0, 0.0, 0.0};
        const double *sw = s_w + lofs + (j * KP + tq) * 16 + fl;
#pragma unroll
        for (int c = 0; c < CH; ++c)
          v[j] = mfma4(ta[sl][c], WL ? sw[4 * (s0 + c) * 16] : wa[sl][WL ? 0 : c], v[j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else if constexpr (VR && !(WL || NKS <= 16)) {
      // J > 4 at K = 128 (W from L2): a runtime loop over the sources, each
      // source's V tile a 4-chunk pipeline of 8 MFMAs with the next chunk's TW
      // and W operands in flight (the last chunk prefetches source j + 1's
      // first), written to the VST slab as soon as it is formed -- the fully
      // unrolled form crashes or spills (CP above); the inline loads left one
      // L2 round trip per source exposed (J = 8, K = 128: 6.85 ms)
      slab_fence0();   // the previous tile's last reads before these writes
      constexpr int CH = 8, CPS = NKS / CH;
      double ta[2][CH], wa[2][CH];
      auto ld = [&](int j, int s0, int sl) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          ta[sl][c] = buf_ld<0>(buf_rsrc(a.TW + t0), vo_tw, (unsigned)((j * KP + 4 * (s0 + c)) * a.Tp) * 8u);
          wa[sl][c] = a.Wkf[lofs + ((size_t)j * KP + tq + 4 * (s0 + c)) * a.Fp + f];
        }
      };
      ld(0, 0, 0);
#pragma unroll 1
      for (int j = 0; j < J; ++j) {
        d4 vj = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int c = 0; c < CPS; ++c) {
          const int sl = c & 1;
          if (c + 1 < CPS)
            ld(j, (c + 1) * CH, sl ^ 1);
          else if (j + 1 < J)
            ld(j + 1, 0, sl ^ 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int cc = 0; cc < CH; ++cc) vj = mfma4(ta[sl][cc], wa[sl][cc], vj);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) wrv[i * 4 * S::VGS + (j >> 2) * 64 + (j & 3)] = vj[i];
      }
    } else if constexpr (VR) {
      // source j + 1's TW operands in flight while source j's MFMAs run; the
      // barriers keep the scheduler from hoisting every source's loads (at
      // K = 64 / 128 they alone would fill the register file)
      // (W from L2 at K = 128, J = 8: no prefetch, or the operands alone spill)
      constexpr bool PFS = WL || NKS <= 16;
      double tn[NKS];
#pragma unroll
      for (int s = 0; s < NKS; ++s) tn[s] = twv[0][s];
#pragma unroll
      for (int j = 0; j < J; ++j) {
        double tc[NKS];
#pragma unroll
        for (int s = 0; s < NKS; ++s)
          tc[s] = PFS || j == 0 ? tn[s]
                               : buf_ld<0>(buf_rsrc(a.TW + t0), vo_tw, (unsigned)((j * KP + 4 * s) * a.Tp) * 8u);
        if (PFS && j + 1 < J) {
#pragma unroll
          for (int s = 0; s < NKS; ++s)
            tn[s] = buf_ld<0>(buf_rsrc(a.TW + t0), vo_tw, (unsigned)(((j + 1) * KP + 4 * s) * a.Tp) * 8u);
        }
        __builtin_amdgcn_sched_barrier(0);
        v[j] = d4{0.0, 0.0, 0.0, 0.0};
        const double *sw = s_w + lofs + (j * KP + tq) * 16 + fl;
        const double *gw = a.Wkf + lofs + ((size_t)j * KP + tq) * a.Fp + f;
#pragma unroll
        for (int s = 0; s < NKS; ++s)
          v[j] = mfma4(tc[s], WL ? sw[4 * s * 16] : gw[(size_t)(4 * s) * a.Fp], v[j]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int j = 0; j < ((VR || CP) ? 0 : J); ++j) {
      v[j] = d4{0.0, 0.0, 0.0, 0.0};
      const double *sw = s_w + lofs + (j * KP + tq) * 16 + fl;
      const double *gw = a.Wkf + lofs + ((size_t)j * KP + tq) * a.Fp + f;
      const double *tw = a.TW + ((size_t)j * KP + tq) * a.Tp + t0 + fl;
#pragma unroll
      for (int s = 0; s < NKS; ++s)
        v[j] = mfma4(j < JA ? twv[j < JA ? j : 0][s] : tw[(size_t)(4 * s) * a.Tp],
                     WL ? sw[4 * s * 16] : gw[(size_t)(4 * s) * a.Fp], v[j]);
    }
    if constexpr (VST && (WL || NKS <= 16)) {   // (else written by the loop above)
      slab_fence0();   // the previous tile's last reads before these writes
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < J; ++j) wrv[i * 4 * S::VGS + (j >> 2) * 64 + (j & 3)] = v[j][i];
    }
    const double *cj = s_cj + lofs + fl;
    // the lane's Sigma_x coefficients: LDS (re-read per tile) or, with
    // CJR, the registers loaded once per kernel
    auto cjv = [&](int j, int c) { return CJR ? cjr[j][c] : cj[(j * 4 + c) * 16]; };
    // point i of the lane's four (frame t0 + tq + 4 i): Sigma_x, its guarded
    // inverse, loglik, P = Cx S, N = S Cx S - S, and rho stored; no LDS
    auto pt_valu = [&](int i, double (&P)[8], double (&N)[4]) {
      const int t = t0 + tq + 4 * i;
      const double x00 = cxv[0][i], x11 = cxv[1][i], xr = cxv[2][i], xi = cxv[3][i];
      double V[J];
#pragma unroll
      for (int j = 0; j < J; ++j) V[j] = VST ? wrv[i * 4 * S::VGS + (j >> 2) * 64 + (j & 3)] : v[j][i];
      // Sigma_x = sum_r V_r a_r a_r^H + PSD I   (compute_suff_stat :613-652)
      double d0 = psd, d1 = psd, ore = 0.0, oim = 0.0;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        d0 += cjv(j, 0) * V[j];
        d1 += cjv(j, 1) * V[j];
        ore += cjv(j, 2) * V[j];
        oim += cjv(j, 3) * V[j];
      }
      // inv_herm_mat_2d (signalTools.py:177-194)
      double det = d0 * d1 - (ore * ore + oim * oim);
      const double dg = det + kEps;
      const double sg = dg > 0.0 ? 1.0 : (dg < 0.0 ? -1.0 : 0.0);
      det = sg * fmax(fabs(det), kEps);
      const double rdet = rcp_nr(det);
      const double i0 = d1 * rdet, i1 = d0 * rdet, ior = -ore * rdet, ioi = -oim * rdet;
      if (fvalid && t < a.T) {
        // log(det pi) as mantissa product x 2^exponent (v_frexp_*: 0, inf and
        // NaN pass through the mantissa, so log(lm) gives -inf / inf / NaN as
        // log() would; a negative det, which the guard only lets through for
        // a Sigma_x that is not positive semi-definite, is flagged in xmin)
        const double x = det * M_PI;
        lev += (double)__builtin_amdgcn_frexp_exp(x);
        lm *= __builtin_amdgcn_frexp_mant(x);
        xmin = fmin(xmin, x);
        ll += i0 * x00 + i1 * x11 + 2.0 * (ior * xr + ioi * xi);
      }
      // P = Cx S, N = S Cx S - S = P^H S - S
      P[0] = x00 * i0 + xr * ior + xi * ioi;   // p00r
      P[1] = xi * ior - xr * ioi;              // p00i
      P[2] = x00 * ior + xr * i1;              // p01r
      P[3] = x00 * ioi + xi * i1;              // p01i
      P[4] = xr * i0 + x11 * ior;              // p10r
      P[5] = -xi * i0 - x11 * ioi;             // p10i
      P[6] = xr * ior + xi * ioi + x11 * i1;   // p11r
      P[7] = xr * ioi - xi * ior;              // p11i
      N[0] = P[0] * i0 + (P[4] * ior - P[5] * ioi) - i0;          // n00
      N[1] = (P[2] * ior + P[3] * ioi) + P[6] * i1 - i1;          // n11
      N[2] = P[0] * ior + P[1] * ioi + P[4] * i1 - ior;           // n01r
      N[3] = P[0] * ioi - P[1] * ior - P[5] * i1 - ioi;           // n01i
      // hat_W[j] = mean over the ranks of j of |V^2 a_r^H N a_r + V| (:727-729,
      // :413-414) in the rank-merged form |V^2 (sum_r a_r^H N a_r) / rk + V|
      // (each rank's term is a posterior second moment, >= 0: the two forms
      // differ by rounding), with sum_r a_r^H N a_r = tr(N sum_r a_r a_r^H) from
      // the Sigma_x coefficients; stored as rho = (hat_W / vm^2) vm,
      // vm = max(V, eps): the FB ratio of update_spectral_components
      // (:1521-1575, N1), formed where V is at hand
      // Since V >= 0, rho = |V^2 q + V| / max(V, eps) = |V q + 1| min(V / eps, 1)
      // (q = a^H N a / rk): no reciprocal (the two forms differ by rounding)
      // NF: the factors 2 (the off-diagonal pair) and 1 / rk (a uniform rank)
      // folded into N once per point instead of once per source
      double Nf[4];
      {
        const double ir = RKU ? 1.0 / (double)RKU : 1.0;
        Nf[0] = N[0] * ir;
        Nf[1] = N[1] * ir;
        Nf[2] = N[2] * (2.0 * ir);
        Nf[3] = N[3] * (2.0 * ir);
      }
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const double Vj = V[j];
        double q;
        if constexpr (NF) {
          q = cjv(j, 0) * Nf[0] + cjv(j, 1) * Nf[1] + cjv(j, 2) * Nf[2] + cjv(j, 3) * Nf[3];
          if constexpr (RKU == 0) q *= inv_rk[j];
        } else {
          const double qa = (cjv(j, 0) * N[0] + cjv(j, 1) * N[1]) +
                            2.0 * (cjv(j, 2) * N[2] + cjv(j, 3) * N[3]);
          q = RKU == 1 ? qa : qa * inv_rk[j];
        }
        const double val = fabs(fma(Vj, q, 1.0)) * fmin(Vj * (1.0 / kEps), 1.0);
        if constexpr (SA)
          es_st<2>(val, buf_rsrc(a.hatW + ((size_t)j * a.Tp + t0) * a.Fp), vo_cx,
                               (unsigned)(4 * i * a.Fp) * 8u);
        else
          __builtin_nontemporal_store(val, a.hatW + ((size_t)j * a.Tp + t) * a.Fp + f);
      }
    };
    // point i's MFMA operands -> the wave's slab (reader layout)
    auto pt_write = [&](int i, const double (&P)[8], const double (&N)[4]) {
      if constexpr (VST) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          wpn[0 * 64 + c] = P[c];
          wpn[1 * 64 + c] = P[4 + c];
          wpn[2 * 64 + c] = N[c];
        }
        return;
      }
      double V[J];
#pragma unroll
      for (int j = 0; j < J; ++j) V[j] = v[j][i];
#pragma unroll
      for (int j = 0; j < J; ++j) wr[(j >> 2) * 64 + (j & 3)] = V[j];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        wr[(S::SP + 0) * 64 + c] = P[c];
        wr[(S::SP + 1) * 64 + c] = P[4 + c];
        wr[S::SN * 64 + c] = N[c];
      }
      if constexpr (!RP) {
        int p = 0;
#pragma unroll
        for (int j1 = 0; j1 < J; ++j1)
#pragma unroll
          for (int j2 = j1; j2 < J; ++j2, ++p)
            wr[(S::SV2 + (p >> 2)) * 64 + (p & 3)] = V[j1] * V[j2];
      }
    };
    // SWP (J >= 4): the next point's VALU work sits between this point's slab
    // reads and its MFMAs (J = 4 with the reader-formed pairs: 0.370 -> 0.367
    // ms alone, 0.373 -> 0.3625 with CJR; with the writer-formed pairs it was
    // neutral; at J > 4 the unpipelined form also tripped ROCm 7.2's
    // AGPR-copy rewrite pass)
    constexpr bool SWP = J >= 4;

    auto slab_fence = [&]() {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // the slab's operands of the 4 bin groups in flight at once, then the
    // MFMAs (read -> wait -> MFMA one at a time left the LDS latency exposed);
    // with SWP the next point's VALU work sits between the reads and the
    // MFMAs (its slab writes after them)
    auto mfma_pass = [&](int i, auto between) {
      if constexpr (VST) {
        // the bin groups in two halves (half the operands live)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          double w[2][Q], pn[2][3];
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) {
            const int g = 2 * hh + g2;
#pragma unroll
            for (int e = 0; e < Q; ++e) w[g2][e] = rdq[(4 * i + g) * S::VGS + vro[e]];
#pragma unroll
            for (int q = 0; q < 3; ++q) pn[g2][q] = rpn[g * S::PGS + q * 64];
          }
          __builtin_amdgcn_sched_barrier(0);
          if (hh == 0) {
            between();
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) {
            const int g = 2 * hh + g2;
#pragma unroll
            for (int vg = 0; vg < NVG; ++vg) {
              xacc[g][vg][0] = mfma44(w[g2][4 * vg], pn[g2][0], xacc[g][vg][0]);
              xacc[g][vg][1] = mfma44(w[g2][4 * vg], pn[g2][1], xacc[g][vg][1]);
            }
#pragma unroll
            for (int h = 0; h < NPG; ++h)
              if (rp_live<J>(h))
                pacc[g][h] = mfma44(w[g2][rp_base<Q>(h)] * w[g2][(rp_base<Q>(h) + rp_d<Q>(h)) & (Q - 1)],
                                    pn[g2][2], pacc[g][h]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        return;
      }
      if constexpr (RP) {
        // rotated sources W_e, then P lo / hi and N, of the 4 bin groups
        double w[4][Q], pn[4][3];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
          for (int e = 0; e < Q; ++e) w[g][e] = rdq[g * S::GS + vro[e]];
#pragma unroll
          for (int q = 0; q < 3; ++q) pn[g][q] = rd[g * S::GS + (S::SP + q) * 64];
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SWP) {
          between();
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
          for (int vg = 0; vg < NVG; ++vg) {
            xacc[g][vg][0] = mfma44(w[g][4 * vg], pn[g][0], xacc[g][vg][0]);
            xacc[g][vg][1] = mfma44(w[g][4 * vg], pn[g][1], xacc[g][vg][1]);
          }
#pragma unroll
          for (int h = 0; h < NPG; ++h)
            if (rp_live<J>(h))
              pacc[g][h] = mfma44(w[g][rp_base<Q>(h)] * w[g][(rp_base<Q>(h) + rp_d<Q>(h)) & (Q - 1)],
                                  pn[g][2], pacc[g][h]);
        }
        return;
      }
      double opd[4][S::NSET];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int q = 0; q < S::NSET; ++q) opd[g][q] = rd[g * S::GS + q * 64];
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (SWP) {
        between();
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int vg = 0; vg < NVG; ++vg) {
          xacc[g][vg][0] = mfma44(opd[g][vg], opd[g][S::SP], xacc[g][vg][0]);
          xacc[g][vg][1] = mfma44(opd[g][vg], opd[g][S::SP + 1], xacc[g][vg][1]);
        }
#pragma unroll
        for (int h = 0; h < NPG; ++h)
          pacc[g][h] = mfma44(opd[g][S::SV2 + h], opd[g][S::SN], pacc[g][h]);
      }
    };
    if constexpr (SWP) {
      double Pc[8], Nc[4];
      pt_valu(0, Pc, Nc);
      pt_write(0, Pc, Nc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        slab_fence();   // point i's slab writes land before the cross-lane reads
        double Pn[8], Nn[4];
        mfma_pass(i, [&]() {
          if (i < 3) pt_valu(i + 1, Pn, Nn);
          if (CXE && i == 2 && tt + 4 < te) load_cx(tt + 4, cxv);
        });
        slab_fence();   // point i + 1's writes must not overtake point i's reads
        if (i < 3) pt_write(i + 1, Pn, Nn);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double P[8], N[4];
        pt_valu(i, P, N);
        pt_write(i, P, N);
        slab_fence();   // the slab writes land before the cross-lane reads
        mfma_pass(i, []() {});
        slab_fence();   // the next point's writes must not overtake these reads
      }
    }
    // keep lm in [0.5, 1): at most 4 factors >= 0.5 were multiplied in
    lev += (double)__builtin_amdgcn_frexp_exp(lm);
    lm = __builtin_amdgcn_frexp_mant(lm);
  }
  ll += (log(lm) + lev * M_LN2) + (xmin < 0.0 ? NAN : 0.0);

  // epilogue: lane (X = m, b, Y = n) holds, per bin group g, the 4x4 blocks
  // D[m][n] of bin f0 + 4g + b: cross (j = m, c = 4h + n), pairs (p = 4h + m, c = n)
  // (VR: pair m of group (base, d); the four waves' sums go through LDS one
  // bin group at a time, [4][NACC][4], to fit the smaller slab allocation)
#pragma unroll
  for (int mm = 1; mm < 64; mm <<= 1) ll += __shfl_xor(ll, mm, 64);
  int tide = tid;   // (launder: see tidp)
  asm volatile("" : "+v"(tide));
  const int lanee = tide & 63, wve = tide >> 6;
  if constexpr (VR) {
    static_assert(4 * NACC * 4 <= 4 * S::SLAB, "VR epilogue fits the slabs");
    const int m = lanee >> 4, bb = (lanee >> 2) & 3, n = lanee & 3;
    double *red = s_slab;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __syncthreads();  // (g = 0: the slabs' last reads; else the previous group's sums)
#pragma unroll
      for (int vg = 0; vg < NVG; ++vg) {
        const int j = 4 * vg + m;
        if (j < J) {
          red[((wve * NACC) + 4 * NP + 8 * j + n) * 4 + bb] = xacc[g][vg][0];
          red[((wve * NACC) + 4 * NP + 8 * j + 4 + n) * 4 + bb] = xacc[g][vg][1];
        }
      }
#pragma unroll
      for (int h = 0; h < NPG; ++h) {
        const int p = rp_pair<J>(h, m);
        if (p >= 0) red[((wve * NACC) + 4 * p + n) * 4 + bb] = pacc[g][h];
      }
      __syncthreads();
      for (int idx = tide; idx < NACC * 4; idx += 256) {
        const int ac = idx >> 2, ff = idx & 3;
        const double x = red[(0 * NACC + ac) * 4 + ff] + red[(1 * NACC + ac) * 4 + ff] +
                         red[(2 * NACC + ac) * 4 + ff] + red[(3 * NACC + ac) * 4 + ff];
        a.part[((size_t)slot * a.Fp + f0 + 4 * g + ff) * NACC + ac] = x;
      }
    }
    if (lanee == 0) s_ll[wve] = ll;
    __syncthreads();
    if (tide == 0)
      a.llpart[slot * a.nft + btile] = ((s_ll[0] + s_ll[1]) + s_ll[2]) + s_ll[3];
  } else {
  __syncthreads();  // s_red aliases the W tile and the slabs
  double *red = s_red + wve * NACC * 16;
  {
    const int m = lanee >> 4, bb = (lanee >> 2) & 3, n = lanee & 3;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int bin = 4 * g + bb;
#pragma unroll
      for (int vg = 0; vg < NVG; ++vg) {
        const int j = 4 * vg + m;
        if (j < J) {
          red[(4 * NP + 8 * j + n) * 16 + bin] = xacc[g][vg][0];
          red[(4 * NP + 8 * j + 4 + n) * 16 + bin] = xacc[g][vg][1];
        }
      }
#pragma unroll
      for (int h = 0; h < NPG; ++h) {
        const int p = rp_pair<J>(h, m);
        if (p >= 0) red[(4 * p + n) * 16 + bin] = pacc[g][h];
      }
    }
  }
  if (lanee == 0) s_ll[wve] = ll;
  __syncthreads();
  for (int idx = tide; idx < NACC * 16; idx += 256) {
    const int ac = idx >> 4, ff = idx & 15;
    const double x = s_red[(0 * NACC + ac) * 16 + ff] + s_red[(1 * NACC + ac) * 16 + ff] +
                     s_red[(2 * NACC + ac) * 16 + ff] + s_red[(3 * NACC + ac) * 16 + ff];
    a.part[((size_t)slot * a.Fp + f0 + ff) * NACC + ac] = x;
  }
  if (tide == 0)
    a.llpart[slot * a.nft + btile] = ((s_ll[0] + s_ll[1]) + s_ll[2]) + s_ll[3];
  }
  // the next segment's prologue rewrites the W tile, the slabs and s_cj that
  // this epilogue (s_red / red alias them) and this segment's tiles read
  __syncthreads();
  if (left <= 0) break;
  // the next bin tile from its first quad-step: this block is the first to
  // meet it, so the segment is the bin tile's slot 0
  const int nq = min(a.es.Q, left);
  ++btile;
  slot = 0;
  tb = a.tbase;
  te = min(tb + 4 * nq, a.ntt);
  left -= nq;
  }  // segments
}

// E-step instantiation chosen from the model structure; `f` receives an
// ETag carrying the template parameters (used for launches and occupancy).
template <int J_, int NKS_, int RKU_, bool CXI_, bool TWI_>
struct ETag {
  static constexpr int J = J_, NKS = NKS_, RKU = RKU_;
  static constexpr bool CXI = CXI_, TWI = TWI_;
};

template <int J, int NKS, int RKU, class F>
static void estep_dispatch_img(const fasst_ctx *c, F &&f) {
  const bool cxi = estep_cxi(c);
  if constexpr (J == 7 && NKS == 32) {   // (never with the Cx image: estep_cxi)
    f(ETag<J, NKS, RKU, false, false>{});
  } else {
    if constexpr (mx_tw_preload<J, NKS>())
      if (estep_twi(c)) {
        if (cxi)
          f(ETag<J, NKS, RKU, true, true>{});
        else
          f(ETag<J, NKS, RKU, false, true>{});
        return;
      }
    if (cxi)
      f(ETag<J, NKS, RKU, true, false>{});
    else
      f(ETag<J, NKS, RKU, false, false>{});
  }
}

template <int J, int NKS, class F>
static void estep_dispatch_r(const fasst_ctx *c, F &&f) {
  bool all1 = true, all2 = true;
  for (int j = 0; j < J; ++j) {
    all1 &= c->rank[j] == 1;
    all2 &= c->rank[j] == 2;
  }
  if (all1)
    estep_dispatch_img<J, NKS, 1>(c, f);
  else if (all2)
    estep_dispatch_img<J, NKS, 2>(c, f);
  else
    estep_dispatch_img<J, NKS, 0>(c, f);
}

template <int J, class F>
static void estep_dispatch_j(const fasst_ctx *c, F &&f) {
  switch (c->KP) {
    case 16: estep_dispatch_r<J, 4>(c, f); break;
    case 32: estep_dispatch_r<J, 8>(c, f); break;
    case 64: estep_dispatch_r<J, 16>(c, f); break;
    default: estep_dispatch_img<J, 32, 0>(c, f); break;   // K up to 128: general ranks only
  }
}

// The two host uses of the model's k_estep_mx<J, ...> instantiation, both in
// the unit that names it.  With e: its launch on c->stream (ny: the frame
// chunks of the chunk grid; the return value says nothing).  Without: its
// dynamic-LDS ceiling raised, then its resident blocks per CU returned.  The
// ceiling is set on the host stub the launch uses: set from another unit it
// would be lost silently.
template <int J>
int estep_mx_j(const fasst_ctx *c, const EArgs *e, int ny) {
  int occ = 1;
  estep_dispatch_j<J>(c, [&](auto tag) {
    using T = decltype(tag);
    constexpr size_t smem = estep_mx_smem<T::J, T::NKS>();
    if (e) {
      const dim3 g = e->es.bal ? dim3(e->es.nb) : dim3(c->nft, ny);
      k_estep_mx<T::J, T::NKS, T::RKU, T::CXI, T::TWI><<<g, 256, smem, c->stream>>>(*e);
      return;
    }
    (void)hipFuncSetAttribute((const void *)k_estep_mx<T::J, T::NKS, T::RKU, T::CXI, T::TWI>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_estep_mx<T::J, T::NKS, T::RKU, T::CXI, T::TWI>, 256,
                                                     smem) != hipSuccess)
      n = 1;
    occ = std::max(1, n);
  });
  return occ;
}

}  // namespace fasst
