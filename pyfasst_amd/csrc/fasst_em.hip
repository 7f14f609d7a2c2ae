// FASST generalized-EM iteration on MI355X (gfx950), FP64 throughout: the model
// configuration (configure_model), the iteration (gem_iteration) and the C ABI.
// This unit holds no kernel: each phase is a unit of its own, reached through
// the host functions of fasst_em.h.
//
// One GEM iteration (audioModel.py:384-428) as gem_iteration issues it, on the
// context's stream unless noted:
//   launch_spectral_prep  k_fwh_t (FW.TW)^T and k_tw_rowsum, forked onto the
//                         side stream beside the E-step   fasst_em_spectral.hip
//   launch_w_old          k_w_from_fb: W = FB.FW          fasst_em_spectral.hip
//   build_inst_A          k_inst_A: 'inst' mixing per bin fasst_em_mix.hip
//   launch_estep_phase    the operand images, k_estep_mx (J <= 8) or k_egen_*
//                         (compute_suff_stat :580-764)    fasst_em_estep.hip,
//                                                         fasst_em_estep_j<J>.hip
//   launch_loglik         k_loglik (:660-664)             fasst_em_estep.hip
//   launch_mix            k_mix, k_mix_inst (update_mix_matrix :766-889)
//                                                         fasst_em_mix.hip
//   spectral_update       k_fb_contract, k_fb_update, k_fw_* (free FW),
//                         k_tw_contract_lds, k_tw_update; or multi_step per
//                         spectral component              fasst_em_spectral.hip
//   launch_renorm         k_renorm_stats / _apply / _final (renormalize_parameters
//                         :1980-2040)                     fasst_em_renorm.hip
// With the fused tail (fast_tail) launch_loglik and launch_renorm give way to
// k_renorm_scales / _rows and the next iteration's W on the side stream inside
// spectral_update, then launch_renorm_tail (k_renorm_tail); the next iteration
// of the batch then skips launch_w_old and, with prep, launch_spectral_prep.
// The fused tail's launch_mix runs on the side stream beside k_fb_contract.
#include "fasst_em.h"
#include "fasst_device.h"

#include <cmath>
#include <cstring>

namespace fasst {

static thread_local std::string g_err;
void set_error(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

// ---------------------------------------------------------------- profiling
static const char *kKernelNames[fasst_ctx::kNK] = {
    "k_w_from_fb", "k_fwh_t", "k_inst_A", "k_estep", "k_loglik", "k_mix",
    "k_mix_inst", "k_fb_contract", "k_fb_update", "k_tw_contract", "k_renorm", "k_tw_update",
    "k_fw_update", "k_tw_rowsum", "k_renorm_tail", "k_tw_statediv", "k_tw_decode",
    "k_sf_gemm", "k_sf_prod", "k_sf_ratio", "k_sf_update", "k_sf_renorm", "k_sf_wiener",
    "k_sf_other", "k_sf_hatw", "k_sf_energy", "k_sf_bary", "k_sf_sparsify",
    "k_sfw_scale", "k_sfw_dgemm2", "k_sfw_update", "k_sfw_renorm"};

// after a device sync: fold the recorded event pairs into the averages
static void prof_collect(fasst_ctx *c) {
  if (!c->prof) return;
  for (int i = 0; i < fasst_ctx::kNK; ++i)
    for (int q = 0; q < fasst_ctx::kProfRing; ++q) {
      if (!c->used[i][q]) continue;
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, c->ev0[i][q], c->ev1[i][q]) == hipSuccess) {
        c->prof_ms[i] += ms;
        c->prof_cnt[i] += 1;
      }
      c->used[i][q] = 0;
    }
}

// Split count c in [1, max_split] for a launch of unit * c equal blocks on
// `cap` resident slots: maximises the filled fraction of the last round
// (unit c / (cap ceil(unit c / cap))), preferring fewer splits within 1.5%.
static int best_split(long unit, long cap, int max_split) {
  max_split = std::max(1, max_split);
  auto eff = [&](int k) {
    const long blocks = unit * k;
    const long rounds = (blocks + cap - 1) / cap;
    return (double)blocks / (double)(rounds * cap);
  };
  double best = 0.0;
  for (int k = 1; k <= max_split; ++k) best = std::max(best, eff(k));
  for (int k = 1; k <= max_split; ++k)
    if (eff(k) >= best - 0.015) return k;
  return 1;
}

int configure_model(fasst_ctx *c, int J, const int *rank, const int *K, const int *convj) {
  if (J < 1 || J > kMaxJ) {
    set_error("J=%d outside the HIP path (1..%d sources)", J, kMaxJ);
    return FASST_ERR_UNSUPPORTED;
  }
  sf_release(c);   // a single-factor model replaces a two-factor one
  int R = 0, kmax = 0;
  for (int j = 0; j < J; ++j) {
    if (rank[j] < 1 || K[j] < 1) {
      set_error("bad rank/K for source %d", j);
      return FASST_ERR_SHAPE;
    }
    R += rank[j];
    kmax = std::max(kmax, K[j]);
  }
  if (R > kMaxR || kmax > kMaxKP) {
    set_error("total rank %d (max %d) / K %d (max %d) outside the HIP path", R, kMaxR, kmax,
              kMaxKP);
    return FASST_ERR_UNSUPPORTED;
  }
  if (int st = spectral_lds_limits()) return st;
  if (int st = estep_lds_limits()) return st;
  if (int st = mix_lds_limits()) return st;
  c->J = J;
  c->R = R;
  c->convm = 0;
  for (int j = 0; j < J; ++j)
    if (convj[j]) c->convm |= 1u << j;
  // conv: every source 'conv' (per-bin mixing update); otherwise the 'inst'
  // update runs over the free 'inst' sources with the rest held fixed
  const int conv = c->convm == (1u << J) - 1u ? 1 : 0;
  c->conv = conv;
  // the E-step addresses TW through a raw buffer resource with 32-bit byte
  // offsets (j KP + 4 s) Tp 8 (k_estep_mx's SA form)
  {
    const int KPc = kmax <= 16 ? 16 : (kmax <= 32 ? 32 : (kmax <= 64 ? 64 : 128));
    if ((size_t)J * KPc * c->Tp * sizeof(double) >= (1ull << 31)) {
      set_error("J %d x K %d x T %d: the TW plane passes the E-step's 2 GB buffer offsets", J,
                KPc, c->T);
      return FASST_ERR_UNSUPPORTED;
    }
  }
  c->KP = kmax <= 16 ? 16 : (kmax <= 32 ? 32 : (kmax <= 64 ? 64 : 128));
  c->roff[0] = 0;
  for (int j = 0; j < J; ++j) {
    c->rank[j] = rank[j];
    c->K[j] = K[j];
    c->roff[j + 1] = c->roff[j] + rank[j];
    c->spat_free[j] = c->fb_free[j] = c->tw_free[j] = 1;
    c->fw_free[j] = 0;
    c->nblk[j] = 1;   // one spectral component per source until fasst_set_blocks
    c->kb[j][0] = 0;
    c->kb[j][1] = K[j];
    c->bfb[j][0] = c->btw[j][0] = 1;
    c->bfw[j][0] = 0;
    c->soff[j] = j;
  }
  c->soff[J] = c->nslot = J;
  c->maxblk = 1;
  c->multi = 0;
  for (int j = 0; j < kMaxJ; ++j)
    for (int b = 0; b < kMaxBlk; ++b) {
      c->tb[j][b].release();
      c->tbl[j][b] = c->btb[j][b] = 0;
    }
  c->anytb = 0;
  for (int j = 0; j < kMaxJ; ++j) c->twc[j] = c->twc_free[j] = 0;
  c->anytwc = 0;
  c->nsrc = 0;
  c->lambda = 0.0;
  c->nseq = 0;
  const int Fp = c->Fp, Tp = c->Tp, KP = c->KP;
  // Launch shapes sized to whole rounds of resident blocks (a partial last
  // round idles most of the chip): E-step blocks = f tiles x frame chunks,
  // FB waves = bin-tile pairs x sources x frame chunks, TW waves = frame-tile
  // pairs x sources x bin chunks.
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess ||
      ncu <= 0)
    ncu = 256;
  const long cap_e = (long)estep_occupancy(c) * ncu;
  // (measured at C3: chunks of >= ~40 frame tiles keep the E-step's per-block
  // prologue/epilogue small; the contractions tolerate finer splits)
  c->nchunk_e = best_split(c->nft, cap_e, c->ntt / 40);
  if (const char *v = getenv("FASST_NCHUNK_E")) c->nchunk_e = std::max(1, std::min(atoi(v), c->ntt));
  c->tpc_e = (c->ntt + c->nchunk_e - 1) / c->nchunk_e;
  c->nchunk_e = (c->ntt + c->tpc_e - 1) / c->tpc_e;
  // The single-pass E-step's schedule (k_estep_mx, J <= 8; fasst_esched.h).
  // FASST_ESTEP_SCHED=chunk | balanced picks it (read here, once per
  // configuration, like FASST_NCHUNK_E), FASST_ESTEP_NB sets the
  // balanced schedule's block count.  Balanced: one round of resident blocks,
  // each at least kEsMinUnits quad-steps (the per-segment prologue / epilogue
  // stays small, as with the chunks of >= 40 frame tiles above) but never
  // fewer blocks than bin tiles.
  c->esched = ESched{};
  c->esched.nbt = c->nft;
  c->esched.nslot = c->nchunk_e;
  {
    // (an explicit FASST_NCHUNK_E asks for the chunk grid)
    bool bal = kEsBalancedDefault && !getenv("FASST_NCHUNK_E");
    if (const char *v = getenv("FASST_ESTEP_SCHED")) bal = !strcmp(v, "balanced");
    const long long Q = (c->ntt + 3) / 4, U = (long long)c->nft * Q;
    if (bal && J <= 8 && U < (1ll << 30)) {
      long long nb = std::min(U, std::max<long long>(c->nft, std::min<long long>(cap_e, U / kEsMinUnits)));
      if (const char *v = getenv("FASST_ESTEP_NB")) nb = atoll(v);
      nb = std::max(1ll, std::min(nb, U));
      c->esched.bal = 1;
      c->esched.nb = (int)nb;
      c->esched.Q = (int)Q;
      c->esched.nslot = es_max_slots(c->nft, (int)Q, (int)nb);
    }
  }
  const long cap_b = (long)contract_occupancy(c) * ncu;
  c->nchunk_b = best_split((long)((c->nft + kFPW - 1) / kFPW) * J, cap_b, c->ntt / 32);
  if (const char *v = getenv("FASST_NCHUNK_B")) c->nchunk_b = std::max(1, std::min(atoi(v), c->ntt));
  c->tpc_b = (c->ntt + c->nchunk_b - 1) / c->nchunk_b;
  c->nchunk_b = (c->ntt + c->tpc_b - 1) / c->tpc_b;
  // (the bin split also multiplies k_tw_update's reduction: a fixed, small
  // split measured best at C3)
  c->nsplit_t = std::max(1, std::min(4, c->nft / 32));
  int tw_units = 0, tw_tiles = 0;
  const long cap_t = (long)twl_occupancy(c, false, &tw_units, &tw_tiles) * ncu;
  if ((long)tw_units * J * c->nsplit_t < cap_t)
    c->nsplit_t = best_split((long)tw_units * J, cap_t, c->nft / 16);
  if (const char *v = getenv("FASST_NSPLIT_T")) c->nsplit_t = std::max(1, std::min(atoi(v), c->nft));
  c->fpc_t = (c->nft + c->nsplit_t - 1) / c->nsplit_t;
  c->nsplit_t = (c->nft + c->fpc_t - 1) / c->fpc_t;
  // k_tw_contract_lds's schedule (the single-component path; fasst_twsched.h).
  // FASST_TWC_SCHED=grid | balanced picks it (read here, once per
  // configuration), FASST_TWC_NB sets the balanced schedule's block count:
  // by default one round of resident blocks.
  c->twsched = TwSched{};
  c->twsched.nslot = c->nsplit_t;
  long cap_tb = 0;
  {
    // (an explicit FASST_NSPLIT_T asks for the grid)
    bool bal = kTwcBalancedDefault && !getenv("FASST_NSPLIT_T");
    if (const char *v = getenv("FASST_TWC_SCHED")) bal = !strcmp(v, "balanced");
    // (k_tw_update's 64-frame blocks each lie inside one frame group)
    if (bal && tw_tiles % 4 == 0 && (long long)J * tw_units * c->nft < (1ll << 30)) {
      cap_tb = (long)twl_occupancy(c, true, &tw_units, &tw_tiles) * ncu;
      long long nb = cap_tb;
      if (const char *v = getenv("FASST_TWC_NB")) nb = atoll(v);
      c->twsched = tws_make(J, tw_units, 16 * tw_tiles, c->nft, nb);
    }
  }
  if (getenv("FASST_VERBOSE"))
    fprintf(stderr,
            "fasst: %d CUs; estep %d %s, %d slots (cap %ld blocks); fb %d chunks (cap %ld); tw %d "
            "%s, %d slots (cap %ld)\n",
            ncu, c->esched.bal ? c->esched.nb : c->nchunk_e,
            c->esched.bal ? "balanced blocks" : "chunks", c->esched.nslot, cap_e, c->nchunk_b, cap_b,
            c->twsched.bal ? c->twsched.nb : c->nsplit_t, c->twsched.bal ? "persistent blocks" : "splits",
            c->twsched.nslot, c->twsched.bal ? cap_tb : cap_t);
  const int NP = J * (J + 1) / 2;
  c->nacc = 4 * NP + 8 * J;
  int st;
#define ALLOC(buf, n) \
  if ((st = c->buf.alloc(n)) != FASST_OK) return st
  ALLOC(FB, (size_t)J * Fp * KP);
  ALLOC(FW, (size_t)J * KP * KP);
  ALLOC(TW, (size_t)J * KP * Tp);
  ALLOC(Wkf, (size_t)J * KP * Fp);
  ALLOC(Wkf_new, (size_t)J * KP * Fp);
  ALLOC(Wfk_new, (size_t)J * Fp * KP);
  ALLOC(FWHt, (size_t)J * Tp * KP);
  ALLOC(hatW, (size_t)J * Tp * Fp);
  ALLOC(A, (size_t)R * 2 * Fp);
  ALLOC(Pinst, (size_t)R * 2);
  // (+8 chunks: the interleaved E-step / FB ranges round their chunks up)
  ALLOC(epart, (size_t)(c->esched.nslot + 8) * Fp * c->nacc);
  ALLOC(llpart, (size_t)(c->esched.nslot + 8) * c->nft);
  ALLOC(bnum, (size_t)(c->nchunk_b + 8) * J * Fp * KP);
  // FW update (free FW only, allocated with the model so set_spectral may switch it on)
  ALLOC(gden, (size_t)c->nchunk_b * J * Fp * KP);
  ALLOC(TWt, (size_t)J * Tp * KP);
  ALLOC(pnum, (size_t)((c->F + fw_fpc(c) - 1) / fw_fpc(c)) * J * KP * KP);
  ALLOC(pden, (size_t)((c->F + fw_fpc(c) - 1) / fw_fpc(c)) * J * KP * KP);
  // (the multi-block path keeps the static split whatever the schedule)
  const int tslots = std::max(c->nsplit_t, c->twsched.nslot);
  ALLOC(tnum, (size_t)tslots * J * Tp * KP);
  ALLOC(tden, (size_t)tslots * J * Tp * KP);
  ALLOC(rss, conv ? 0 : (size_t)Fp * R * R);
  ALLOC(rxs, conv ? 0 : (size_t)Fp * 2 * R);
  ALLOC(flags, kNFlags);
  ALLOC(hsum, (size_t)J * KP);
  // renormalisation chunks (every stage-2 block re-reduces all stage-1
  // partials, so more chunks measured slower at C3)
  c->nchunk_r = std::max(1, std::min(64, std::min((c->T + 255) / 256, (c->F + 15) / 16)));
  ALLOC(rscal, (size_t)J * (2 + 2 * KP));
  ALLOC(rpmax, (size_t)J * c->nchunk_r * KP);
  ALLOC(rpe, (size_t)J * c->nchunk_r);
  ALLOC(rtpart, (size_t)kMaxSlot * c->nchunk_r);
  c->ntb = (Tp + 63) / 64;
  ALLOC(rpmax2, (size_t)J * c->nft * KP);
  ALLOC(rtpart2, (size_t)kMaxSlot * c->ntb);
  ALLOC(Wkf_next, (size_t)J * KP * Fp);
  ALLOC(hpart, (size_t)J * KP * c->ntb);
  if (J > 8 && KP > 32) {   // the two-pass E-step's scratch: V_j, N, P planes and per-tile logliks
    ALLOC(vgen, (size_t)J * Tp * Fp);
    ALLOC(npgen, (size_t)12 * Tp * Fp);
    ALLOC(lgen, (size_t)c->ntt * c->nft);
  } else {
    c->vgen.release();
    c->npgen.release();
    c->lgen.release();
  }
  c->w_ready = c->prep_ready = 0;
  // the E-step's operand images follow the model: the TW image its J and KP
  // (re-allocated by the next iteration), the Cx image whether it is read
  c->twp.release();
  if (!estep_cxi(c)) {
    c->cxp.release();
    c->cxp_valid = false;
  }
#undef ALLOC
  c->configured = 1;
  return FASST_OK;
}

static void update_multi(fasst_ctx *c) {
  c->anytb = 0;
  for (int j = 0; j < c->J; ++j)
    for (int b = 0; b < c->nblk[j]; ++b) c->anytb |= c->tbl[j][b] > 0;
  c->multi = c->maxblk > 1 || c->lambda > 0.0 || c->anytb;
}

// gem_iteration's fused renormalisation tail (§3.3a of DESIGN.md; see
// k_renorm_scales), the default for the structures it covers: one spectral
// component per source (!multi), no time blobs (!anytb), no free FW.  The
// context's ftail (FASST_FAST_TAIL, read at creation) selects the form:
//   0  the unfused k_renorm_stats / _apply / _final (the A/B reference);
//   1  the fused tail: k_fb_update's stage-1 statistics, k_renorm_scales /
//      _rows and the next W on the side stream beside the TW contraction,
//      the TW rescale inside k_tw_update, k_renorm_tail;
//   2  (default) as 1, and at KP <= 64 k_tw_update also forms the next
//      iteration's (FW.TW)^T and TW row-sum partials (reduced into hsum by
//      k_renorm_tail), so the next iteration of the batch skips
//      launch_spectral_prep.
// Every form is tested against the others and the oracle, halted batches
// included (tests/test_gpu_fast_tail.py).
static bool fast_tail(const fasst_ctx *c) {
  if (!c->ftail || c->multi || c->anytb || c->anytwc) return false;
  for (int j = 0; j < c->J; ++j)
    if (c->fw_free[j]) return false;
  return true;
}

// One GEM iteration, all launches asynchronous on c->stream.
static int gem_iteration(fasst_ctx *c, const double *psd_dev, double *ll_dev, double omega,
                         int iter) {
  const int J = c->J;
  if (!c->conv) {
    // a free 'conv' component next to other components: the reference's conv
    // solve (audioModel.py:856-857) passes the full hat_Rss[f].T against the
    // free components' right-hand side only, and np.linalg.solve raises
    for (int j = 0; j < J; ++j)
      if ((c->convm >> j & 1u) && c->spat_free[j]) {
        set_error("spatial component %d is 'conv' and free next to other components: the "
                  "reference's mixing solve (audioModel.py:856-857) raises for this structure",
                  j);
        return FASST_ERR_UNSUPPORTED;
      }
  }
  // (FW.TW)^T and the TW row sums depend only on the previous iteration's
  // parameters: forked onto the side stream beside the E-step (unless the
  // previous iteration's fused tail in the same batch formed them)
  const bool prep_ready = c->prep_ready;
  c->prep_ready = 0;
  int st = prep_ready ? FASST_OK : launch_spectral_prep(c, true);
  if (st) return st;
  const bool w_ready = c->w_ready;   // (the previous iteration's fused tail formed W)
  c->w_ready = 0;
  if (!w_ready && (st = launch_w_old(c))) return st;
  st = build_inst_A(c);
  if (st) return st;
  if ((st = launch_estep_phase(c, psd_dev, prep_ready))) return st;
  if (!prep_ready) FASST_HIP(hipStreamWaitEvent(c->stream, c->ev_join, 0));  // hsum, FWHt below
  const bool ft = fast_tail(c);
  if (!ft && (st = launch_loglik(c, ll_dev))) return st;   // (fused tail: summed by k_renorm_tail)
  // mixing update (update_mix_matrix, :766-889).  (On the side stream beside
  // the TW contraction instead, after the FB update: k_mix stretched to 0.18
  // ms and took 23 us from the TW contraction and 14 us from the FB
  // contraction for the 30 us it left the critical path; profiles/r6_ab_mix_side.txt)
  // With the fused tail it runs on the side stream beside the HBM-bound FB
  // contraction, which reads nothing it writes: forked here, launched before
  // the contraction so its one-wave blocks take their slots first.  The side
  // stream's k_renorm_scales, the first reader of the new mixing parameters,
  // follows it in stream order; spectral_update puts k_fb_update, the first
  // kernel that moves a parameter, behind ev_mix, so a singular solve halts
  // the iteration's updates as it does on one stream.
  const bool mix_side = ft && c->mix_side;
  if (mix_side) {
    FASST_HIP(hipEventRecord(c->ev_mixf, c->stream));
    FASST_HIP(hipStreamWaitEvent(c->aux, c->ev_mixf, 0));
  }
  if ((st = launch_mix(c, mix_side ? c->aux : c->stream))) return st;
  if (mix_side) FASST_HIP(hipEventRecord(c->ev_mix, c->aux));
  if ((st = spectral_update(c, omega, ft))) return st;
  if (!ft) return launch_renorm(c, iter);
  const bool prep = c->ftail >= 2 && c->KP <= 64;   // (spectral_update's k_tw_update formed FWHt)
  if ((st = launch_renorm_tail(c, ll_dev, iter, prep))) return st;
  std::swap(c->Wkf.p, c->Wkf_next.p);
  c->w_ready = 1;
  c->prep_ready = prep;
  return FASST_OK;
}

}  // namespace fasst

using namespace fasst;

// ============================================================================ C ABI
extern "C" {

const char *fasst_last_error(void) { return fasst::g_err.c_str(); }

int fasst_abi_version(void) { return FASST_ABI_VERSION; }

int fasst_estep_partition(int nbt, int Q, int nb, long long *lo, int *first, int *nseg,
                          int *max_slots) {
  if (nbt < 1 || Q < 1 || nb < 1 || (long long)nbt * Q >= (1ll << 30) || nb > (long long)nbt * Q) {
    set_error("fasst_estep_partition: need 1 <= nb <= nbt Q < 2^30 (nbt=%d Q=%d nb=%d)", nbt, Q, nb);
    return FASST_ERR_SHAPE;
  }
  const long long U = (long long)nbt * Q;
  if (lo)
    for (int b = 0; b <= nb; ++b) lo[b] = es_lo(b, U, nb);
  for (int bt = 0; bt < nbt; ++bt) {
    if (first) first[bt] = es_first(bt, Q, nbt, nb);
    if (nseg) nseg[bt] = es_nseg(bt, Q, nbt, nb);
  }
  if (max_slots) *max_slots = es_max_slots(nbt, Q, nb);
  return FASST_OK;
}

int fasst_device_count(int *n) {
  FASST_HIP(hipGetDeviceCount(n));
  return FASST_OK;
}

int fasst_create(int device, int F, int T, fasst_ctx **out) {
  if (!out || F < 1 || T < 1) {
    set_error("fasst_create: bad arguments F=%d T=%d", F, T);
    return FASST_ERR_SHAPE;
  }
  int ndev = 0;
  FASST_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) {
    set_error("fasst_create: device %d not present (%d visible)", device, ndev);
    return FASST_ERR_DEVICE;
  }
  DeviceGuard g(device);
  fasst_ctx *c = new fasst_ctx();
  c->device = device;
  c->F = F;
  c->T = T;
  c->Fp = round_up(F, kTile);
  c->Tp = round_up(T, kTile);
  c->nft = c->Fp / kTile;
  c->ntt = c->Tp / kTile;
  if (const char *v = getenv("FASST_FAST_TAIL")) c->ftail = atoi(v);
  if (const char *v = getenv("FASST_MIX_SIDE")) c->mix_side = atoi(v) != 0;
  if (const char *v = getenv("FASST_ESTEP_IMG"))
    c->eimg = !strcmp(v, "cx") ? 1 : (!strcmp(v, "tw") ? 2 : (!strcmp(v, "0") ? 0 : 3));
  int st = FASST_OK;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_tail, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_scales, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_rows, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_mixf, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_mix, hipEventDisableTiming) != hipSuccess) {
    set_error("hipStreamCreate / hipEventCreate failed");
    st = FASST_ERR_DEVICE;
  }
  if (!st) st = c->cx.alloc((size_t)4 * c->Tp * c->Fp);
  if (!st && hipHostMalloc((void **)&c->h_flags, kNFlags * sizeof(int)) != hipSuccess)
    st = FASST_ERR_OOM;
  if (!st && hipHostMalloc((void **)&c->h_ll, 64 * sizeof(double)) != hipSuccess) st = FASST_ERR_OOM;
  if (st) {
    fasst_destroy(c);
    return st;
  }
  *out = c;
  return FASST_OK;
}

int fasst_configure_types(fasst_ctx *c, int J, const int *rank, const int *K,
                          const int *mix_conv) {
  if (!c || !rank || !K || !mix_conv) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  return configure_model(c, J, rank, K, mix_conv);
}

int fasst_configure(fasst_ctx *c, int J, const int *rank, const int *K, int mix_conv) {
  if (!c || !rank || !K) return FASST_ERR_SHAPE;
  if (J < 1 || J > kMaxJ) return configure_model(c, J, rank, K, nullptr);
  int types[kMaxJ];
  for (int j = 0; j < J; ++j) types[j] = mix_conv ? 1 : 0;
  DeviceGuard g(c->device);
  return configure_model(c, J, rank, K, types);
}

int fasst_destroy(fasst_ctx *c) {
  if (!c) return FASST_OK;
  {
    DeviceGuard g(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->aux) (void)hipStreamSynchronize(c->aux);
    sf_release(c);
    if (c->h_flags) (void)hipHostFree(c->h_flags);
    if (c->h_ll) (void)hipHostFree(c->h_ll);
    c->cx.release();
    c->cxp.release();
    c->twp.release();
    c->X.release();
    c->FB.release();
    c->FW.release();
    c->TW.release();
    c->Wkf.release();
    c->Wkf_new.release();
    c->Wfk_new.release();
    c->FWHt.release();
    c->hatW.release();
    c->A.release();
    c->Pinst.release();
    c->epart.release();
    c->llpart.release();
    c->bnum.release();
    c->tnum.release();
    c->tden.release();
    c->psd.release();
    c->ll.release();
    c->rss.release();
    c->rxs.release();
    c->flags.release();
    c->hsum.release();
    c->rscal.release();
    c->rpmax.release();
    c->rpe.release();
    c->rtpart.release();
    c->rpmax2.release();
    c->rtpart2.release();
    c->hpart.release();
    c->vgen.release();
    c->npgen.release();
    c->lgen.release();
    c->Wkf_next.release();
    c->mplanes.release();
    c->bden.release();
    for (int i = 0; i < fasst_ctx::kNK; ++i) {
      for (int q = 0; q < fasst_ctx::kProfRing; ++q) {
        if (c->ev0[i][q]) (void)hipEventDestroy(c->ev0[i][q]);
        if (c->ev1[i][q]) (void)hipEventDestroy(c->ev1[i][q]);
      }
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_tail) (void)hipEventDestroy(c->ev_tail);
    if (c->ev_scales) (void)hipEventDestroy(c->ev_scales);
    if (c->ev_rows) (void)hipEventDestroy(c->ev_rows);
    if (c->ev_mixf) (void)hipEventDestroy(c->ev_mixf);
    if (c->ev_mix) (void)hipEventDestroy(c->ev_mix);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->stream) (void)hipStreamDestroy(c->stream);
  }
  delete c;
  return FASST_OK;
}

static int need_model(fasst_ctx *c, int j) {
  if (!c || !c->configured) {
    set_error("context not configured");
    return FASST_ERR_SHAPE;
  }
  if (j < 0 || j >= c->J) {
    set_error("component %d out of range (J=%d)", j, c->J);
    return FASST_ERR_SHAPE;
  }
  return FASST_OK;
}

int fasst_set_spatial(fasst_ctx *c, int j, const double *params, int free_) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  c->spat_free[j] = free_ ? 1 : 0;
  const int r0 = c->roff[j], nr = c->rank[j];
  const double2 *p = reinterpret_cast<const double2 *>(params);
  if (c->convm >> j & 1u) {
    // params [r][C][F] -> A[r][c][f] (row pitch Fp)
    FASST_TRY(c->A.at((size_t)2 * r0 * c->Fp, (size_t)2 * nr * c->Fp)
                  .put_rows(p, (size_t)nr * 2, c->F, c->F, c->Fp, c->stream));
  } else {
    // params [C][r] -> Pinst[r][c]
    std::vector<double2> tmp((size_t)nr * 2);
    for (int r = 0; r < nr; ++r)
      for (int ch = 0; ch < 2; ++ch) tmp[(size_t)r * 2 + ch] = p[(size_t)ch * nr + r];
    FASST_TRY(c->Pinst.at(2 * r0, tmp.size()).put(tmp.data(), tmp.size(), c->stream));
  }
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_get_spatial(fasst_ctx *c, int j, double *params) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  const int r0 = c->roff[j], nr = c->rank[j];
  double2 *p = reinterpret_cast<double2 *>(params);
  if (c->convm >> j & 1u) {
    FASST_TRY(c->A.at((size_t)2 * r0 * c->Fp, (size_t)2 * nr * c->Fp)
                  .get_rows(p, (size_t)nr * 2, c->F, c->F, c->Fp, c->stream));
    FASST_HIP(hipStreamSynchronize(c->stream));
  } else {
    std::vector<double2> tmp((size_t)nr * 2);
    FASST_TRY(c->Pinst.at(2 * r0, tmp.size()).get(tmp.data(), tmp.size(), c->stream));
    FASST_HIP(hipStreamSynchronize(c->stream));
    for (int r = 0; r < nr; ++r)
      for (int ch = 0; ch < 2; ++ch) p[(size_t)ch * nr + r] = tmp[(size_t)r * 2 + ch];
  }
  return FASST_OK;
}

int fasst_set_fw_prior(fasst_ctx *c, int j, int fw_free) {
  int st = need_model(c, j);
  if (st) return st;

  c->fw_free[j] = fw_free ? 1 : 0;
  if (c->nblk[j] == 1) c->bfw[j][0] = c->fw_free[j];
  return FASST_OK;
}

int fasst_set_blocks(fasst_ctx *c, int j, int nblk, const int *kb, const int *fb_free,
                     const int *fw_free, const int *tw_free) {
  int st = need_model(c, j);
  if (st) return st;
  if (nblk < 1 || nblk > kMaxBlk || !kb || !fb_free || !fw_free || !tw_free) {
    set_error("source %d: %d spectral components (1..%d on the HIP path)", j, nblk, kMaxBlk);
    return nblk > kMaxBlk ? FASST_ERR_UNSUPPORTED : FASST_ERR_SHAPE;
  }
  if (kb[0] != 0 || kb[nblk] != c->K[j]) {
    set_error("source %d: component blocks must cover its %d columns", j, c->K[j]);
    return FASST_ERR_SHAPE;
  }
  for (int b = 0; b < nblk; ++b)
    if (kb[b + 1] <= kb[b]) {
      set_error("source %d: empty or unordered component block %d", j, b);
      return FASST_ERR_SHAPE;
    }
  int nslot = 0, maxblk = 0;
  for (int i = 0; i < c->J; ++i) {
    const int n = i == j ? nblk : c->nblk[i];
    nslot += n;
    maxblk = std::max(maxblk, n);
  }
  if (nslot > kMaxSlot) {
    set_error("%d spectral components in all (max %d on the HIP path)", nslot, kMaxSlot);
    return FASST_ERR_UNSUPPORTED;
  }
  DeviceGuard g(c->device);
  if (maxblk > 1) {
    const size_t plane = (size_t)c->J * c->Tp * c->Fp;
    if (c->mplanes.n < 5 * plane && (st = c->mplanes.alloc(5 * plane))) return st;
    const size_t nb = (size_t)c->nchunk_b * c->J * c->Fp * c->KP;
    if (c->bden.n < nb && (st = c->bden.alloc(nb))) return st;
  }
  bool same = c->nblk[j] == nblk;
  for (int b = 0; same && b <= nblk; ++b) same = c->kb[j][b] == kb[b];
  c->nblk[j] = nblk;
  if (nblk > 1 && c->twc[j]) {   // a discrete-state TW needs the source's only component
    c->twc[j] = c->twc_free[j] = c->anytwc = 0;
    for (int i = 0; i < c->J; ++i) c->anytwc |= c->twc[i] != 0;
  }
  for (int b = 0; b <= nblk; ++b) c->kb[j][b] = kb[b];
  bool fbf = false, twf = false, fwf = false;
  for (int b = 0; b < nblk; ++b) {
    c->bfb[j][b] = fb_free[b] ? 1 : 0;
    c->bfw[j][b] = fw_free[b] ? 1 : 0;
    c->btw[j][b] = tw_free[b] ? 1 : 0;
    fbf |= c->bfb[j][b] != 0;
    fwf |= c->bfw[j][b] != 0;
    twf |= c->btw[j][b] != 0;
  }
  c->fb_free[j] = fbf;
  c->fw_free[j] = fwf;
  c->tw_free[j] = twf;
  c->soff[0] = 0;
  for (int i = 0; i < c->J; ++i) c->soff[i + 1] = c->soff[i] + c->nblk[i];
  c->nslot = nslot;
  c->maxblk = maxblk;
  if (!same)   // the blocks moved: their time blobs go (an unchanged layout,
               // e.g. the per-iteration re-upload, keeps them and their buffers)
    for (int b = 0; b < kMaxBlk; ++b) {
      c->tb[j][b].release();
      c->tbl[j][b] = c->btb[j][b] = 0;
    }
  update_multi(c);
  return FASST_OK;
}

int fasst_set_corr(fasst_ctx *c, double lambda, int nseq, const int *seq_j, const int *seq_b) {
  int st = need_model(c, 0);
  if (st) return st;
  if (!(lambda >= 0.0) || (lambda > 0.0 && (nseq < 1 || nseq > kMaxSlot || !seq_j || !seq_b))) {
    set_error("fasst_set_corr: lambda %g with %d components", lambda, nseq);
    return FASST_ERR_SHAPE;
  }
  if (lambda > 0.0) {
    int seen[kMaxJ][kMaxBlk] = {{0}};
    for (int q = 0; q < nseq; ++q) {
      const int j = seq_j[q], b = seq_b[q];
      if (j < 0 || j >= c->J || b < 0 || b >= c->nblk[j] || seen[j][b]++) {
        set_error("fasst_set_corr: bad component (%d, %d) at position %d", j, b, q);
        return FASST_ERR_SHAPE;
      }
      c->seq_j[q] = j;
      c->seq_b[q] = b;
    }
    if (nseq != c->nslot) {
      set_error("fasst_set_corr: %d components given, the model has %d", nseq, c->nslot);
      return FASST_ERR_SHAPE;
    }
    DeviceGuard g(c->device);
    const size_t plane = (size_t)c->J * c->Tp * c->Fp;
    if (c->mplanes.n < 5 * plane && (st = c->mplanes.alloc(5 * plane))) return st;
    const size_t nb = (size_t)c->nchunk_b * c->J * c->Fp * c->KP;
    if (c->bden.n < nb && (st = c->bden.alloc(nb))) return st;
  }
  c->lambda = lambda;
  c->nseq = lambda > 0.0 ? nseq : 0;
  update_multi(c);
  return FASST_OK;
}

int fasst_set_tb(fasst_ctx *c, int j, int b, int L, const double *TW, const double *TB,
                 int tb_free) {
  int st = need_model(c, j);
  if (st) return st;
  if (b < 0 || b >= c->nblk[j] || L < 0 || L > kMaxTB || (L > 0 && (!TW || !TB))) {
    set_error("fasst_set_tb: source %d component %d with %d time blobs (1..%d)", j, b, L, kMaxTB);
    return L > kMaxTB ? FASST_ERR_UNSUPPORTED : FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  if (L == 0) {
    c->tb[j][b].release();
    c->tbl[j][b] = c->btb[j][b] = 0;
    update_multi(c);
    return FASST_OK;
  }
  const int kbw = c->kb[j][b + 1] - c->kb[j][b];
  const TBLayout o = tb_layout(kbw, L, c->Tp);
  const size_t plane = (size_t)c->J * c->Tp * c->Fp;
  if (c->mplanes.n < 6 * plane && (st = c->mplanes.alloc(6 * plane))) return st;
  const size_t nb = (size_t)c->nchunk_b * c->J * c->Fp * c->KP;
  if (c->bden.n < nb && (st = c->bden.alloc(nb))) return st;
  // a buffer large enough is reused (no hipMalloc / device-wide sync on the
  // per-iteration re-upload); either way it is zero-filled: TB's padding
  // frames stay 0
  if (c->tb[j][b].n < o.n) {
    if ((st = c->tb[j][b].alloc(o.n))) return st;
  } else {
    FASST_TRY(c->tb[j][b].zero(o.n, c->stream));
  }
  FASST_TRY(c->tb[j][b].at(o.tws).put(TW, (size_t)kbw * L, c->stream));
  FASST_TRY(c->tb[j][b].at(o.tb).put_rows(TB, L, c->T, c->T, c->Tp, c->stream));
  c->tbl[j][b] = L;
  c->btb[j][b] = tb_free ? 1 : 0;
  if (c->twc[j]) {   // time blobs and a discrete-state TW exclude each other (:1736-1742)
    c->twc[j] = c->twc_free[j] = c->anytwc = 0;
    for (int i = 0; i < c->J; ++i) c->anytwc |= c->twc[i] != 0;
  }
  update_multi(c);
  c->halt = nullptr;
  if ((st = launch_tb_set(c, j, b))) return st;   // H = TW TB into the block's rows
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_get_tb(fasst_ctx *c, int j, int b, double *TW, double *TB) {
  int st = need_model(c, j);
  if (st) return st;
  if (b < 0 || b >= c->nblk[j] || c->tbl[j][b] == 0) {
    set_error("fasst_get_tb: source %d component %d has no time blobs", j, b);
    return FASST_ERR_SHAPE;
  }
  DeviceGuard g(c->device);
  const int kbw = c->kb[j][b + 1] - c->kb[j][b], L = c->tbl[j][b];
  const TBLayout o = tb_layout(kbw, L, c->Tp);
  if (TW)
    FASST_TRY(c->tb[j][b].at(o.tws).get(TW, (size_t)kbw * L, c->stream));
  if (TB) FASST_TRY(c->tb[j][b].at(o.tb).get_rows(TB, L, c->T, c->T, c->Tp, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_set_spectral(fasst_ctx *c, int j, const double *FB, const double *FW, const double *TW,
                       int fb_free, int tw_free) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  const int K = c->K[j], KP = c->KP;
  c->fb_free[j] = fb_free ? 1 : 0;
  c->tw_free[j] = tw_free ? 1 : 0;
  if (c->nblk[j] == 1) {
    c->bfb[j][0] = c->fb_free[j];
    c->btw[j][0] = c->tw_free[j];
  }
  // source j's rows of the padded images FB [Fp][KP], FW [KP][KP], TW [KP][Tp]
  const DSpan<double> fb = c->FB.at((size_t)j * c->Fp * KP, (size_t)c->Fp * KP),
                      fw = c->FW.at((size_t)j * KP * KP, (size_t)KP * KP),
                      tw = c->TW.at((size_t)j * KP * c->Tp, (size_t)KP * c->Tp);
  FASST_TRY(fw.zero(fw.n, c->stream));
  FASST_TRY(fb.put_rows(FB, c->F, K, K, KP, c->stream));
  FASST_TRY(fw.put_rows(FW, K, K, K, KP, c->stream));
  FASST_TRY(tw.put_rows(TW, K, c->T, c->T, c->Tp, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_get_spectral(fasst_ctx *c, int j, double *FB, double *FW, double *TW) {
  int st = need_model(c, j);
  if (st) return st;
  DeviceGuard g(c->device);
  const int K = c->K[j], KP = c->KP;
  if (FB)
    FASST_TRY(c->FB.at((size_t)j * c->Fp * KP, (size_t)c->Fp * KP)
                  .get_rows(FB, c->F, K, K, KP, c->stream));
  if (FW)
    FASST_TRY(c->FW.at((size_t)j * KP * KP, (size_t)KP * KP).get_rows(FW, K, K, K, KP, c->stream));
  if (TW)
    FASST_TRY(c->TW.at((size_t)j * KP * c->Tp, (size_t)KP * c->Tp)
                  .get_rows(TW, K, c->T, c->T, c->Tp, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_spectral_update(fasst_ctx *c, const double *hat_W, double omega) {
  int st = need_model(c, 0);
  if (st) return st;
  if (!hat_W) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  const size_t n = (size_t)c->J * c->F * c->T;
  DBuf<double> dh;
  if ((st = dh.alloc_uninit(n))) return st;
  FASST_TRY(dh.put(hat_W, n, c->stream));
  FASST_TRY(c->flags.zero(kNFlags, c->stream));
  c->halt = nullptr;
  if ((st = launch_spectral_prep(c, false)) || (st = launch_w_old(c))) return st;
  FASST_TRY(c->hatW.zero((size_t)c->J * c->Tp * c->Fp, c->stream));
  if ((st = launch_rho_from_hatw(c, dh.p)) || (st = spectral_update(c, omega))) return st;
  FASST_HIP(hipStreamSynchronize(c->stream));
  return FASST_OK;
}

int fasst_renormalize(fasst_ctx *c, int *restart_mask) {
  int st = need_model(c, 0);
  if (st) return st;
  DeviceGuard g(c->device);
  FASST_TRY(c->flags.zero(kNFlags, c->stream));
  c->halt = nullptr;
  st = launch_renorm(c, 0);
  if (st) return st;
  FASST_TRY(c->flags.get(c->h_flags, kNFlags, c->stream));
  FASST_HIP(hipStreamSynchronize(c->stream));
  int mask = 0;
  for (int sl = 0; sl < c->nslot; ++sl)
    if (c->h_flags[1 + sl]) mask |= 1 << sl;
  if (restart_mask) *restart_mask = mask;
  return FASST_OK;
}

int fasst_run(fasst_ctx *c, int n_iter, const double *psd, double omega, double *logliks,
              int *restart_mask, int *iters_done) {
  int st = need_model(c, 0);
  if (st) return st;
  if (n_iter < 0 || (n_iter > 0 && (!psd || !logliks))) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  if (iters_done) *iters_done = 0;
  if (restart_mask) *restart_mask = 0;
  if (n_iter == 0) return FASST_OK;
  if (c->psd_cap < n_iter) {
    if ((st = c->psd.alloc((size_t)n_iter * c->Fp))) return st;
    c->psd_cap = n_iter;
  }
  if (c->ll_cap < n_iter) {
    if ((st = c->ll.alloc(n_iter))) return st;
    c->ll_cap = n_iter;
  }
  FASST_TRY(c->psd.zero((size_t)n_iter * c->Fp, c->stream));
  FASST_TRY(c->psd.at(0).put_rows(psd, n_iter, c->F, c->F, c->Fp, c->stream));
  FASST_TRY(c->flags.zero(kNFlags, c->stream));
  // Without profiling the whole batch is enqueued at once: a flag raised in
  // iteration i halts every later kernel on the device (HALT_GUARD), and the
  // host reads the flags once at the end.  Profiling keeps one sync per
  // iteration so the per-kernel events can be folded.
  c->halt = c->flags.p + kFlagHalt;
  c->w_ready = c->prep_ready = 0;
  const int sync_every = c->prof ? fasst_ctx::kProfRing : n_iter;
  int done = 0;
  for (int it = 0; it < n_iter; ++it) {
    c->pslot = it % fasst_ctx::kProfRing;
    st = gem_iteration(c, c->psd.p + (size_t)it * c->Fp, c->ll.p + it, omega, it);
    if (st) {
      c->halt = nullptr;
      return st;
    }
    if ((it + 1) % sync_every && it + 1 < n_iter) continue;
    FASST_TRY(c->flags.get(c->h_flags, kNFlags, c->stream));
    FASST_HIP(hipStreamSynchronize(c->stream));
    prof_collect(c);
    done = it + 1;
    if (c->h_flags[kFlagHalt] || c->h_flags[0]) break;
  }
  c->halt = nullptr;
  // a halted batch skipped its later iterations' kernels while the host still
  // swapped the fused tail's W buffers: rebuild W = FB.FW from the parameters
  if (c->w_ready && (c->h_flags[kFlagHalt] || c->h_flags[0])) {
    if ((st = launch_w_old(c))) return st;
    FASST_HIP(hipStreamSynchronize(c->stream));
  }
  c->w_ready = c->prep_ready = 0;
  if (c->h_flags[0]) {
    set_error("Singular Matrix");
    return FASST_ERR_SINGULAR;
  }
  int mask = 0;
  for (int sl = 0; sl < c->nslot; ++sl)
    if (c->h_flags[1 + sl]) mask |= 1 << sl;
  if (mask) done = c->h_flags[kFlagIter] + 1;
  if (iters_done) *iters_done = done;
  FASST_TRY(c->ll.get(logliks, done));
  if (mask) {
    if (restart_mask) *restart_mask = mask;
    return FASST_TW_RESTART;
  }
  return FASST_OK;
}

int fasst_set_profiling(fasst_ctx *c, int on) {
  if (!c) return FASST_ERR_SHAPE;
  DeviceGuard g(c->device);
  if (on && !c->ev0[0][0])
    for (int i = 0; i < fasst_ctx::kNK; ++i)
      for (int q = 0; q < fasst_ctx::kProfRing; ++q) {
        FASST_HIP(hipEventCreate(&c->ev0[i][q]));
        FASST_HIP(hipEventCreate(&c->ev1[i][q]));
      }
  c->prof = on ? 1 : 0;
  c->pslot = 0;
  for (int i = 0; i < fasst_ctx::kNK; ++i) {
    c->prof_ms[i] = 0.0;
    c->prof_cnt[i] = 0;
    for (int q = 0; q < fasst_ctx::kProfRing; ++q) c->used[i][q] = 0;
  }
  return FASST_OK;
}

int fasst_kernel_times(fasst_ctx *c, double *avg_ms, long *counts, int nk) {
  if (!c || !avg_ms) return FASST_ERR_SHAPE;
  for (int i = 0; i < nk && i < fasst_ctx::kNK; ++i) {
    avg_ms[i] = c->prof_cnt[i] ? c->prof_ms[i] / (double)c->prof_cnt[i] : 0.0;
    if (counts) counts[i] = c->prof_cnt[i];
  }
  return fasst_ctx::kNK;
}

const char *fasst_kernel_name(int i) {
  return (i >= 0 && i < fasst_ctx::kNK) ? kKernelNames[i] : "";
}

}  // extern "C"
