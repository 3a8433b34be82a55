// bwgr_amd/csrc/uvb_host.hip.h -- the host entries of the per-trait ridge fits on a resident int8 panel (bwgr_uvbeta, bwgr_uvbeta2), of the
// same fits on a small dense design (bwgr_uvbeta_dense), and of X B (bwgr_panel_xb).  Part of bwgr_hip.hip, after mrr_host.hip.h (the launch
// constants it shares with mrr are mtfit_host.hip.h's); it defines no kernel.  The fits' host algebra is uvb_tail.h, what they do to Y and Z before a kernel runs traits.h.
// ------------------------------------------------------------------------------------------------
// solver1x / UVBETA, solver1xF / FUVBETA, xsolver1xF / XFUVBETA, zsolver1xF / ZFUVBETA
// (src/RcppEigen20230423.cpp:1410-1443, :1506-1515, :1613-1646, :1709-1753, :1771-1816): the engine of uvb.hip.h
//   once:       k_uvb_setup, k_uvb_cols(TrXSX) per group of 64 traits
//   per sweep:  order (host std::shuffle, cumulative) -> k_permute_cols, then for every group with a trait still running:
//               k_mrr_gram -> [k_uvb_pass(b-1 | b), k_uvb_solve(b)] for every block -> k_uvb_pass(last | -) -> k_uvb_rows, k_uvb_cols;
//               one copy of every group's sums -> (host: mu, ve, vb, lambda, cnv, who stops) -> k_uvb_mu_shift
// ------------------------------------------------------------------------------------------------
// The plan, decided here and nowhere else (bwgr_debug_uvb_plan exposes it to the CPU tests): the groups, the solve's LDS (as many of a
// solve workgroup's Gram matrices as fit beside u), the pass's grid, and the element counts of the call's device arrays.
static constexpr int UVB_SHIFT_WG = 1024;     // workgroups of k_uvb_mu_shift per trait at most, 256 rows each per trip
static inline int64_t uvb_pass_grid(int64_t ld) { return std::min<int64_t>(ld / 64, UVB_PASS_WG); }
static inline int64_t uvb_shift_grid(int64_t n) { return std::min<int64_t>((n + TAIL_THREADS - 1) / TAIL_THREADS, UVB_SHIFT_WG); }
static inline int64_t uvb_xb_grid(int64_t n) { return (n + TAIL_THREADS - 1) / TAIL_THREADS; }
struct UvbPlan {
  int64_t groups, nblk, kpad; int ngl, G, nsolve; size_t lds_solve, lds_pass;
  size_t x_bytes, n_gram, n_zm, n_rows, n_cols, n_part, n_dB, n_tpart, n_res, n_slot, n_bout, n_xb;   // element counts
  size_t ws_bytes;
};
// npat_max: the most patterns any group has; npat_total: the patterns of all groups.  Negative: their bounds (every trait its own pattern),
// which is what is known before Y has been read.
static UvbPlan uvb_plan(int64_t n, int64_t ld, int64_t p, int64_t k, size_t x_bytes, int64_t npat_max, int64_t npat_total, bool want_xb) {
  UvbPlan pl;
  if (npat_max < 0) npat_max = std::min<int64_t>(k, UVB_W);
  if (npat_total < 0) npat_total = k;
  pl.groups = (k + UVB_W - 1) / UVB_W; pl.kpad = pl.groups * UVB_W; pl.nblk = (p + MRR_MB - 1) / MRR_MB;
  pl.nsolve = UVB_W / UVB_ST;
  pl.ngl = (int)std::min<size_t>((size_t)UVB_ST, (MRR_LDS_MAX - uvb_solve_lds(0)) / ((size_t)UVB_GSTR * 4));
  pl.lds_solve = uvb_solve_lds(pl.ngl); pl.lds_pass = UVB_PASS_LDS;
  pl.G = (int)uvb_pass_grid(ld);
  pl.x_bytes = x_bytes;
  pl.n_gram = (size_t)pl.nblk * (size_t)npat_max * MRR_MB * MRR_MB;      // int32: one group's block Gram matrices, rebuilt per sweep and group
  pl.n_zm = (size_t)npat_total * ld;                                      // bytes: the row masks k_mrr_gram ANDs with
  pl.n_rows = (size_t)pl.kpad * ld;                                       // doubles: y, e
  pl.n_cols = (size_t)pl.kpad * p;                                        // doubles: S, XX, tilde, b
  pl.n_part = (size_t)pl.G * (MRR_MB + 1) * UVB_W; pl.n_dB = (size_t)(MRR_MB + 1) * UVB_W;
  pl.n_tpart = (size_t)UVB_NP * 3 * UVB_W; pl.n_res = (size_t)pl.kpad * 6;
  pl.n_slot = (size_t)pl.groups * pl.nsolve * pl.ngl;
  pl.n_bout = (size_t)p * k; pl.n_xb = want_xb ? (size_t)n * k : 0;
  pl.ws_bytes = x_bytes + 4 * (size_t)p + 4 * std::max<size_t>(pl.n_gram, 1) + std::max<size_t>(pl.n_zm, 1) + 8 * (size_t)pl.groups * ld + 8 * (2 * pl.n_rows + 4 * pl.n_cols + pl.n_part + pl.n_dB + pl.n_tpart + pl.n_res) +
                8 * 2 * (size_t)pl.kpad /* db2, mu0 */ + sizeof(UvbTrait) * (size_t)pl.kpad + 4 * pl.n_slot + 8 * (pl.n_bout + pl.n_xb);
  return pl;
}
extern "C" int bwgr_debug_uvb_plan(int64_t n, int64_t p, int64_t k, int64_t out[BWGR_UVB_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "uvb plan: null pointer");
  if (n < 1 || p < 1 || k < 1) return fail(BWGR_EINVAL, "uvb plan: n = %lld, p = %lld, k = %lld (each at least 1)", (long long)n, (long long)p, (long long)k);
  const int64_t ld = (n + 127) / 128 * 128;
  const UvbPlan pl = uvb_plan(n, ld, p, k, (size_t)ld * p, -1, -1, true);
  out[0] = UVB_W; out[1] = pl.groups; out[2] = UVB_ST; out[3] = pl.ngl; out[4] = (int64_t)pl.lds_solve; out[5] = (int64_t)pl.lds_pass;
  out[6] = pl.G; out[7] = (int64_t)pl.ws_bytes;
  return BWGR_OK;
}

// (bwgr_uvbeta_dense's plan, above its first user: the dense leg of bwgr_uvbeta2 carves its LDS up by the same rule)
// The plan, decided here and nowhere else (bwgr_debug_uvbd_plan exposes it to the CPU tests): whether a trait's residual lives in its
// workgroup's LDS or in a global workspace, the workgroup size, the dynamic LDS bytes and the bytes of that workspace.
struct UvbdPlan { int64_t lds_rows; bool e_in_lds; int threads; size_t lds_bytes, ws_bytes; };
static UvbdPlan uvbd_plan(int64_t n, int64_t q, int64_t k) {
  (void)q;   // (the per-column values live in global memory: the LDS carve-up does not depend on q)
  UvbdPlan pl;
  pl.lds_rows = (int64_t)((UVBD_LDS_MAX - UVBD_LDS_FIXED) / sizeof(double));
  pl.e_in_lds = n <= pl.lds_rows;
  pl.threads = (int)std::min<int64_t>(UVBD_TMAX, (n + 63) / 64 * 64);   // one row per thread up to 1024 rows, whole waves
  pl.lds_bytes = UVBD_LDS_FIXED + (pl.e_in_lds ? sizeof(double) * (size_t)n : 0);
  pl.ws_bytes = pl.e_in_lds ? 0 : sizeof(double) * (size_t)n * (size_t)k;
  return pl;
}

// ---- what bwgr_uvbeta, bwgr_uvbeta2 and bwgr_uvbeta_dense do alike ----
static int uvb_accept(const char *who, int64_t k, int64_t kmax, int variant, int maxit) {
  if (k < 1 || k > kmax) return fail(BWGR_EINVAL, "%s: k = %lld traits (at least 1)", who, (long long)k);
  if (variant < BWGR_UVB_D || variant > BWGR_UVB_Z) return fail(BWGR_EINVAL, "%s: unknown variant %d (0 solver1x, 1 solver1xF, 2 xsolver1xF, 3 zsolver1xF)", who, variant);
  if (maxit < 0) return fail(BWGR_EINVAL, "%s: maxit = %d", who, maxit);
  return BWGR_OK;
}
// Y on the traits' own rows, as submat_f / subvec_f select them (:1495-1503): nt, mu (:1413), the centred y (:1414), vy = y'y / (nt - 1) (:1419;
// y'Y = y'y: sum y = 0).  A trait without a row is an all-NaN trait: a zero column, no sweeps (:1510, :1713, :1811)
static int uvb_read(const char *who, const double *Y, int64_t n, int64_t k, int64_t ld, int64_t ycols, TraitSet &S) {
  S = read_traits(Y, n, k, ld, ycols, RowRule::NotOne);
  if (S.bad >= 0) return fail(BWGR_EINVAL, "%s: trait %lld has one observed row (the variances divide by n - 1)", who, (long long)S.bad);
  return BWGR_OK;
}
static int z_unpadded(const char *who, const double *Z, int64_t n, int64_t q, int64_t ldz, std::vector<double> &Zc) {
  int64_t r = 0, j = 0;
  if (!compact_z(Z, n, q, ldz, Zc, &r, &j)) return fail(BWGR_EINVAL, "%s: Z[%lld, %lld] is not finite", who, (long long)r, (long long)j);
  return BWGR_OK;
}

// What bwgr_uvbeta2 adds to a fit: solver2x (:1446-1493) -- in every sweep the dense design Z is walked first (k_uvb2_leg, uvb2.hip.h), then
// the panel, against one residual; each design has its own lambda and variance update; the dense design's outputs are b1 and vb1.
// bwgr_uvbeta2 makes it before the fit, so what is copied from and to asynchronously here outlives the fit's holder.
struct UvDenseLeg {
  const double *Z; int64_t q, ldz; double *b1, *vb1;   // the call's
  std::vector<double> Zc;                               // Z without its padding
  CumulativeOrder order{0};
  std::vector<Uvb2Trait> tr;
  std::vector<double> sums, trx;                        // [trait][UVB2_NLEG] of the last sweep; TrXSX1
  hipStream_t st = nullptr; int64_t n = 0, ld = 0, k = 0, kpad = 0;
  UvbdPlan dpl;                                         // the leg's launch shape is uvbd_plan's
  Uvb2Args da; double *Zd = nullptr; Uvb2Trait *trd = nullptr; int32_t *ordd = nullptr;

  int accept(const char *who, int64_t n_) {
    if (q < 1 || q > 0x7FFFFF00ll || ldz < n_)
      return fail(BWGR_EINVAL, "%s: q = %lld columns of Z, ldz = %lld (q at least 1 and at most 2147483392, the int32 column ids; ldz at least n = %lld)", who, (long long)q, (long long)ldz, (long long)n_);
    order = CumulativeOrder((size_t)q);
    return z_unpadded(who, Z, n_, q, ldz, Zc);
  }
  // the dense design's arrays: Z, the traits' per-column values, the leg's sums (the caller asks bufs.failed())
  void alloc(DevBufs &bufs, hipStream_t st_, int64_t n_, int64_t ld_, int64_t k_, int64_t kpad_) {
    st = st_; n = n_; ld = ld_; k = k_; kpad = kpad_;
    dpl = uvbd_plan(n, q, k);
    tr.resize((size_t)kpad); sums.resize((size_t)kpad * UVB2_NLEG); trx.resize((size_t)kpad);
    const size_t nc = (size_t)kpad * (size_t)q;
    Zd = bufs.get<double>((size_t)n * (size_t)q);
    double *c1 = bufs.get<double>(5 * nc);
    da.trx = bufs.get<double>((size_t)kpad); da.leg = bufs.get<double>((size_t)kpad * UVB2_NLEG);
    trd = bufs.get<Uvb2Trait>((size_t)kpad); ordd = bufs.get<int32_t>((size_t)q);
    da.Z = Zd; da.n = n; da.q = q; da.ld = ld; da.tr = trd; da.order = ordd;
    da.zbar = c1; da.XX = c1 + nc; da.tilde = c1 + 2 * nc; da.b = c1 + 3 * nc; da.dlt = c1 + 4 * nc;
  }
  // y, e and the masks are the fit's; a trait's mask is its pattern's, in its group's masks (at zm_off[group])
  int upload(const double *yd, double *ed, const uint8_t *zmd, const std::vector<UvbTrait> &ftr, const std::vector<size_t> &zm_off) {
    da.y = yd; da.e = ed; da.zm = zmd;
    for (int64_t t = 0; t < kpad; ++t) {
      Uvb2Trait &u = tr[(size_t)t];
      u.lam = 0.0; u.nt = ftr[(size_t)t].nt; u.moff = (int64_t)(zm_off[(size_t)(t / UVB_W)] + (size_t)ftr[(size_t)t].pat * (size_t)ld); u.run = 0; u.pad_ = 0;
    }
    const size_t nc = (size_t)kpad * (size_t)q;
    HIPCHK(h2d(st, Zd, Zc.data(), Zc.size()));
    HIPCHK(h2d(st, trd, tr.data(), tr.size()));
    HIPCHK(zero(st, da.zbar, 5 * nc));                                                                  // b_1 = 0, :1458
    HIPCHK(zero(st, da.trx, (size_t)kpad));
    HIPCHK(zero(st, da.leg, (size_t)kpad * UVB2_NLEG));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvb2_leg<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)UVBD_LDS_MAX));
    return BWGR_OK;
  }
  // (after the copies of y and the masks, on the same stream)
  int setup() {
    hipLaunchKernelGGL(k_uvb2_setup, dim3((unsigned)k), dim3(dpl.threads), UVBD_LDS_FIXED, st, da);
    HIPCHK(hipMemcpyAsync(trx.data(), da.trx, sizeof(double) * kpad, hipMemcpyDeviceToHost, st));
    return BWGR_OK;
  }
  int stage(int sweep, const std::vector<UvbState> &T) {
    for (int64_t t = 0; t < k; ++t) { tr[(size_t)t].lam = T[(size_t)t].lam1; tr[(size_t)t].run = (T[(size_t)t].active && !T[(size_t)t].skip1) ? 1 : 0; }
    HIPCHK(h2d(st, ordd, order.next(sweep).data(), (size_t)q));                                            // :1468 (cumulative, as there)
    HIPCHK(h2d(st, trd, tr.data(), tr.size()));
    return BWGR_OK;
  }
  // the dense leg (:1470-1473) of group g's running traits, in front of the panel's; one workgroup per trait of the group
  void launch(int64_t g) {
    const unsigned kg = (unsigned)std::min<int64_t>(UVB_W, k - g * UVB_W);
    Uvb2Args ga = da;
    const size_t o1 = (size_t)g * UVB_W * (size_t)q, orow = (size_t)g * UVB_W * (size_t)ld;
    ga.y += orow; ga.e += orow; ga.tr += g * UVB_W; ga.zbar += o1; ga.XX += o1; ga.tilde += o1; ga.b += o1; ga.dlt += o1; ga.trx += g * UVB_W; ga.leg += (size_t)g * UVB_W * UVB2_NLEG;
    if (dpl.e_in_lds) hipLaunchKernelGGL(k_uvb2_leg<true>, dim3(kg), dim3(dpl.threads), dpl.lds_bytes, st, ga);
    else hipLaunchKernelGGL(k_uvb2_leg<false>, dim3(kg), dim3(dpl.threads), dpl.lds_bytes, st, ga);
  }
  int sums_back() { HIPCHK(hipMemcpyAsync(sums.data(), da.leg, sizeof(double) * kpad * UVB2_NLEG, hipMemcpyDeviceToHost, st)); return BWGR_OK; }
  int results(const std::vector<UvbState> &T) {
    HIPCHK(d2h(st, b1, da.b, sizeof(double) * (size_t)q * (size_t)k));   // ([trait][q] = q x k, column-major)
    if (vb1) for (int64_t t = 0; t < k; ++t) vb1[t] = T[(size_t)t].vb1;
    return BWGR_OK;
  }
};

// A per-trait fit on the device: k traits in groups of 64 over the rows of one panel, with or without a dense leg (null: solver1x and its kin).
// uvb_run makes one after its checks and calls the steps from its loop; every step enqueues on st what it names, in that order.
struct UvFit {
  const char *who; const bwgr_panel *P; const int64_t n, p, ld, k, groups, kpad; const int R, variant, maxit; const double tol, df0; const bool want_xb;
  UvDenseLeg *const leg;
  const hipStream_t st;
  UvbPlan pl;
  TraitSet S;
  std::vector<UvbState> T;
  std::vector<UvbTrait> tr;
  std::vector<unsigned long long> zb;            // per group: the observed-row word of every row
  std::vector<uint8_t> zm;                       // per group and pattern: the row masks k_mrr_gram ANDs with
  std::vector<int> npat, slotpat;                // per group: its patterns -- traits with the same observed rows share one masked Gram
  std::vector<size_t> zm_off;
  CumulativeOrder order;
  std::vector<double> res, db2h, mu0;
  int8_t *Xs = nullptr; int32_t *ordd = nullptr, *gram = nullptr; uint8_t *zmd = nullptr; unsigned long long *zbd = nullptr;
  double *yd = nullptr, *ed = nullptr, *Sd = nullptr, *XXd = nullptr, *tilde = nullptr, *bd = nullptr, *part = nullptr, *dB = nullptr, *tpart = nullptr, *resd = nullptr;
  double *db2 = nullptr, *mu0d = nullptr, *bout = nullptr, *xbd = nullptr;
  UvbTrait *trd = nullptr; int *slotd = nullptr;
  DevBufs bufs;   // last: members go away in reverse order, so the holder's wait for the stream comes before any vector above is gone

  UvFit(const char *who_, const bwgr_panel *P_, int64_t k_, int variant_, int maxit_, double tol_, double df0_, UvDenseLeg *leg_, bool want_xb_)
      : who(who_), P(P_), n(P_->data->n), p(P_->data->p), ld(P_->data->plan.ld), k(k_), groups((k_ + UVB_W - 1) / UVB_W), kpad(groups * UVB_W), R(P_->data->plan.R),
        variant(variant_), maxit(maxit_), tol(tol_), df0(df0_), want_xb(want_xb_), leg(leg_), st(P_->stream), order((size_t)p), bufs(P_->stream) {}

  // the traits of group g that have rows / that still run
  unsigned long long mask_of(int64_t g, bool running) const {
    unsigned long long m = 0;
    for (int tl = 0; tl < UVB_W; ++tl) {
      const int64_t t = g * UVB_W + tl;
      if (t < k && (running ? T[(size_t)t].active : T[(size_t)t].nt > 0)) m |= 1ull << tl;
    }
    return m;
  }
  // sums over the markers of a group, partials in a fixed order, into resd[g][3 .. 4]
  void cols(int64_t g, int mode, unsigned long long act) {
    const size_t oc = (size_t)g * UVB_W * (size_t)p;
    hipLaunchKernelGGL(k_uvb_cols, dim3(UVB_NP), dim3(256), 0, st, (const double *)(bd + oc), (const double *)(tilde + oc), (const double *)(XXd + oc), p, mode, act, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, UVB_NP, 2 * UVB_W, resd + (size_t)g * 6 * UVB_W + 3 * UVB_W);
  }
  // Y, the groups' row words, patterns and masks, then the plan and the solve workgroups' slots
  int read(const double *Y) {
    CHK(uvb_read(who, Y, n, k, ld, kpad, S));
    T.resize((size_t)k);
    for (int64_t t = 0; t < k; ++t) {
      UvbState &q = T[(size_t)t];
      q.nt = S.nt[(size_t)t]; q.mu = S.mu[(size_t)t]; q.sumy = S.sumy[(size_t)t]; q.vy = S.vy[(size_t)t];
      q.active = q.nt > 0 && maxit > 0;
    }
    const UvbTrait idle = {0.0, 0.0, 0, -1, 0, 0};
    tr.assign((size_t)kpad, idle); zb.resize((size_t)groups * ld); npat.assign((size_t)groups, 0); zm_off.assign((size_t)groups, 0);
    int64_t npat_total = 0;
    for (int64_t g = 0; g < groups; ++g) {
      const int64_t t0 = g * UVB_W;
      const int kg = (int)std::min<int64_t>(UVB_W, k - t0);
      pack_row_bits(S, t0, kg, zb.data() + (size_t)g * ld);
      const Patterns pg = find_patterns(S, t0, t0 + kg);
      npat[(size_t)g] = (int)pg.rep.size(); zm_off[(size_t)g] = zm.size(); npat_total += npat[(size_t)g];
      append_byte_masks(S, pg.rep.data(), npat[(size_t)g], zm);
      for (int tl = 0; tl < kg; ++tl)
        if (pg.id[(size_t)tl] >= 0) { tr[(size_t)(t0 + tl)].nt = S.nt[(size_t)(t0 + tl)]; tr[(size_t)(t0 + tl)].pat = pg.id[(size_t)tl]; }
    }
    // (the int32 pattern Grams sum over at most n rows: n * max|x|^2 < 2^31 holds for every int8 panel, panel_build_gram)
    pl = uvb_plan(n, ld, p, k, P->data->plan.x_bytes, *std::max_element(npat.begin(), npat.end()), npat_total, want_xb);
    slotpat = uvb_slots(tr, {groups, pl.nsolve, pl.ngl, UVB_W, UVB_ST});
    return BWGR_OK;
  }
  int alloc() {
    res.resize(pl.n_res); db2h.resize((size_t)kpad); mu0.assign((size_t)kpad, 0.0);
    Xs = bufs.get<int8_t>(pl.x_bytes);
    ordd = bufs.get<int32_t>((size_t)p); gram = bufs.get<int32_t>(pl.n_gram);
    zmd = bufs.get<uint8_t>(pl.n_zm);   // (= zm.size())
    zbd = bufs.get<unsigned long long>((size_t)groups * ld);
    yd = bufs.get<double>(pl.n_rows); ed = bufs.get<double>(pl.n_rows);
    Sd = bufs.get<double>(pl.n_cols); XXd = bufs.get<double>(pl.n_cols); tilde = bufs.get<double>(pl.n_cols); bd = bufs.get<double>(pl.n_cols);
    part = bufs.get<double>(pl.n_part); dB = bufs.get<double>(pl.n_dB); tpart = bufs.get<double>(pl.n_tpart); resd = bufs.get<double>(pl.n_res);
    db2 = bufs.get<double>((size_t)kpad); mu0d = bufs.get<double>((size_t)kpad);
    trd = bufs.get<UvbTrait>((size_t)kpad);
    slotd = bufs.get<int>(pl.n_slot);
    bout = bufs.get<double>(pl.n_bout); xbd = want_xb ? bufs.get<double>(pl.n_xb) : nullptr;
    if (bufs.failed()) return no_memory(who);
    if (leg) leg->alloc(bufs, st, n, ld, k, kpad);
    return bufs.failed() ? no_memory(who) : BWGR_OK;
  }
  int upload() {
    if (leg) CHK(leg->upload(yd, ed, zmd, tr, zm_off));
    if (!zm.empty()) HIPCHK(h2d(st, zmd, zm.data(), zm.size()));
    HIPCHK(h2d(st, zbd, zb.data(), zb.size()));
    HIPCHK(h2d(st, yd, S.y.data(), pl.n_rows));
    HIPCHK(h2d(st, ed, S.y.data(), pl.n_rows));                                                         // e = y, :1422
    HIPCHK(h2d(st, trd, tr.data(), tr.size()));
    HIPCHK(h2d(st, slotd, slotpat.data(), pl.n_slot));
    HIPCHK(zero(st, bd, pl.n_cols));                                                                    // b = 0, :1421
    HIPCHK(zero(st, dB, pl.n_dB));
    HIPCHK(zero(st, part, pl.n_part));
    HIPCHK(zero(st, tpart, pl.n_tpart));
    HIPCHK(zero(st, resd, pl.n_res));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvb_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvb_pass), hipFuncAttributeMaxDynamicSharedMemorySize, (int)UVB_PASS_LDS));
    return BWGR_OK;
  }
  // S, XX, tilde and TrXSX of every group, the leg's own, then every trait's start values
  int setup() {
    for (int64_t g = 0; g < groups; ++g) {
      const unsigned long long have = mask_of(g, false);
      if (!have) continue;
      const int kg = (int)std::min<int64_t>(UVB_W, k - g * UVB_W);
      const size_t oc = (size_t)g * UVB_W * (size_t)p, orow = (size_t)g * UVB_W * (size_t)ld;
      hipLaunchKernelGGL(k_uvb_setup, dim3((unsigned)pl.nblk), dim3(256), 0, st, (const int8_t *)P->data->X, R, p, ld, (const unsigned long long *)(zbd + (size_t)g * ld),
                         (const double *)(yd + orow), (const UvbTrait *)(trd + g * UVB_W), kg, Sd + oc, XXd + oc, tilde + oc);
      cols(g, 1, have);
    }
    if (leg) CHK(leg->setup());
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, res.data(), resd, sizeof(double) * pl.n_res));
    for (int64_t t = 0; t < k; ++t)
      if (T[(size_t)t].nt != 0.0)
        uvb_start(T[(size_t)t], variant, df0, p, res[(size_t)(t / UVB_W) * 6 * UVB_W + 3 * UVB_W + (size_t)(t % UVB_W)], leg ? &leg->trx[(size_t)t] : nullptr);
    return BWGR_OK;
  }
  // the next sweep's lambdas and who runs it; false: nobody
  bool stage_traits() {
    bool any = false;
    for (int64_t t = 0; t < k; ++t) { tr[(size_t)t].lam = T[(size_t)t].lam; tr[(size_t)t].active = T[(size_t)t].active ? 1 : 0; any = any || T[(size_t)t].active; }
    return any;
  }
  // order -> k_permute_cols, then every group with a trait still running
  int sweep(int s) {
    HIPCHK(h2d(st, ordd, order.next(s).data(), (size_t)p));                                                // :1428 (cumulative, as there)
    HIPCHK(h2d(st, trd, tr.data(), tr.size()));
    hipLaunchKernelGGL(k_permute_cols, dim3(8192), dim3(256), 0, st, (const uint4 *)P->data->X, (uint4 *)Xs, (const int32_t *)ordd, p, P->data->plan.K, (int)((size_t)R / 16));
    HIPCHK(zero(st, db2, (size_t)kpad));
    if (leg) CHK(leg->stage(s, T));
    for (int64_t g = 0; g < groups; ++g) {
      const unsigned long long act = mask_of(g, true);
      if (act) CHK(sweep_group(g, act));
    }
    return BWGR_OK;
  }
  // [the dense leg ->] k_mrr_gram -> [k_uvb_pass(b-1 | b), k_uvb_solve(b)] for every block -> k_uvb_pass(last | -) -> k_uvb_rows, k_uvb_cols
  int sweep_group(int64_t g, unsigned long long act) {
    const size_t oc = (size_t)g * UVB_W * (size_t)p, orow = (size_t)g * UVB_W * (size_t)ld;
    const int ng = npat[(size_t)g];
    const int64_t nblk = pl.nblk;
    const double thr = variant == BWGR_UVB_F ? 0.00001 : 0.0;
    if (leg) leg->launch(g);
    int nsolve = 0;
    for (int sb = 0; sb < pl.nsolve; ++sb) if ((act >> (sb * UVB_ST)) & 0xFFFFull) nsolve = sb + 1;
    hipLaunchKernelGGL(k_mrr_gram, dim3((unsigned)nblk, (unsigned)((ng + 3) / 4)), dim3(256), 0, st, (const int8_t *)Xs, R, p, ld, (const uint8_t *)(zmd + zm_off[(size_t)g]), ng, gram);
    for (int64_t blk = 0; blk <= nblk; ++blk) {
      UvbPassArgs pa; pa.Xs = Xs; pa.R = R; pa.p = p; pa.ld = ld; pa.zb = zbd + (size_t)g * ld; pa.e = ed + orow; pa.dB = dB; pa.part = part;
      pa.prev = blk > 0 ? (int)(blk - 1) : -1; pa.next = blk < nblk ? (int)blk : -1; pa.act = act;
      hipLaunchKernelGGL(k_uvb_pass, dim3(pl.G), dim3(256), pl.lds_pass, st, pa);
      if (blk == nblk) break;
      UvbSolveArgs sa; sa.part = part; sa.G = pl.G; sa.order = ordd; sa.blk = (int)blk; sa.p = p; sa.gram = gram; sa.npat = ng; sa.S = Sd + oc; sa.XX = XXd + oc;
      sa.b = bd + oc; sa.dB = dB; sa.db2 = db2 + g * UVB_W; sa.tr = trd + g * UVB_W; sa.slotpat = slotd + (size_t)g * pl.nsolve * pl.ngl; sa.ngl = pl.ngl; sa.thr = thr;
      hipLaunchKernelGGL(k_uvb_solve, dim3(nsolve), dim3(256), pl.lds_solve, st, sa);
    }
    hipLaunchKernelGGL(k_uvb_rows, dim3(UVB_NP, UVB_W), dim3(256), 0, st, (const double *)(ed + orow), (const double *)(yd + orow), ld, act, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, UVB_NP, 3 * UVB_W, resd + (size_t)g * 6 * UVB_W);
    cols(g, 0, act);
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // the sums back, the tail of every trait that ran (uvb_update), and mu0 off their residuals
  int tail() {
    const double logtol = log10(tol), *lsum = nullptr;
    HIPCHK(hipMemcpyAsync(db2h.data(), db2, sizeof(double) * kpad, hipMemcpyDeviceToHost, st));
    if (leg) { CHK(leg->sums_back()); lsum = leg->sums.data(); }
    HIPCHK(d2h(st, res.data(), resd, sizeof(double) * pl.n_res));
    for (int64_t t = 0; t < k; ++t) {
      mu0[(size_t)t] = 0.0;
      if (!T[(size_t)t].active) continue;
      const double *rg = res.data() + (size_t)(t / UVB_W) * 6 * UVB_W + (size_t)(t % UVB_W);
      const UvbSums sums = {rg[0], rg[UVB_W], rg[2 * UVB_W], rg[3 * UVB_W], rg[4 * UVB_W], db2h[(size_t)t], lsum ? lsum + (size_t)t * UVB2_NLEG : nullptr};
      mu0[(size_t)t] = uvb_update(T[(size_t)t], sums, variant, maxit, logtol, df0, p, lsum ? leg->q : 0);
    }
    HIPCHK(h2d(st, mu0d, mu0.data(), mu0.size()));
    for (int64_t g = 0; g < groups; ++g) {
      unsigned long long ran = 0;
      for (int tl = 0; tl < UVB_W; ++tl) if (tr[(size_t)(g * UVB_W + tl)].active) ran |= 1ull << tl;   // (tr.active still says who ran this sweep)
      if (!ran) continue;
      hipLaunchKernelGGL(k_uvb_mu_shift, dim3((unsigned)uvb_shift_grid(n), UVB_W), dim3(TAIL_THREADS), 0, st, ed + (size_t)g * UVB_W * (size_t)ld,
                         (const unsigned long long *)(zbd + (size_t)g * ld), ld, (int)n, ran, (const double *)(mu0d + g * UVB_W));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // mu0 is rewritten by the next sweep's tail
    return BWGR_OK;
  }
  int results(const UvbOut &out, double *b_out, double *xb_out) {
    for (int64_t g = 0; g < groups; ++g) {
      const int kg = (int)std::min<int64_t>(UVB_W, k - g * UVB_W);
      const size_t oc = (size_t)g * UVB_W * (size_t)p;
      hipLaunchKernelGGL(k_uvb_b_out, dim3((unsigned)std::min<int64_t>((p * kg + 255) / 256, 4096)), dim3(256), 0, st, (const double *)(bd + oc), p, kg, bout + (size_t)g * UVB_W * (size_t)p);
      if (xb_out)
        hipLaunchKernelGGL(k_uvb_xb, dim3((unsigned)uvb_xb_grid(n), (unsigned)((kg + 15) / 16)), dim3(TAIL_THREADS), 0, st, (const int8_t *)P->data->X, R, p, (int)n, (const double *)(bd + oc), kg,
                           xbd + (size_t)g * UVB_W * n);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, b_out, bout, sizeof(double) * pl.n_bout));
    if (xb_out) HIPCHK(d2h(st, xb_out, xbd, sizeof(double) * pl.n_xb));
    if (leg) CHK(leg->results(T));
    for (int64_t t = 0; t < k; ++t) {
      const UvbState &q = T[(size_t)t];
      uvb_result(out, t, q.nt == 0.0, variant, q.mu, q.ve, q.vb, q.vy, q.cnv, q.its);
    }
    return BWGR_OK;
  }
};

// The engine of bwgr_uvbeta and bwgr_uvbeta2 (leg given, variant D only)
static int uvb_run(const char *who, bwgr_panel *P, const double *Y, int64_t k, int variant, int maxit, double tol, double df0, UvDenseLeg *leg, double *b_out,
                   double *mu_out, double *h2_out, double *ve_out, double *vb_out, int *its_out, double *cnv_out, double *xb_out) {
  if (!P || !Y || !b_out || !its_out) return fail(BWGR_EINVAL, "%s: null pointer", who);
  CHK(uvb_accept(who, k, INT64_MAX, variant, maxit));
  if (P->data->is_f32) return fail(BWGR_EINVAL, "%s: the panel holds fp32 genotypes; %s takes int8 panels only", who, who);
  if (leg) CHK(leg->accept(who, P->data->n));
  HIPCHK(hipSetDevice(P->data->device));
  UvFit F(who, P, k, variant, maxit, tol, df0, leg, xb_out != nullptr);
  CHK(F.read(Y));
  CHK(F.alloc());
  CHK(F.upload());
  CHK(F.setup());
  for (int s = 0; s < maxit && F.stage_traits(); ++s) {
    CHK(F.sweep(s));
    CHK(F.tail());
  }
  const UvbOut out = {mu_out, h2_out, ve_out, vb_out, cnv_out, its_out};
  return F.results(out, b_out, xb_out);
}

extern "C" int bwgr_uvbeta(bwgr_panel *P, const double *Y, int64_t k, int variant, int maxit, double tol, double df0, double *b_out, double *mu_out,
                           double *h2_out, double *ve_out, double *vb_out, int *its_out, double *cnv_out, double *xb_out) {
  return uvb_run("uvbeta", P, Y, k, variant, maxit, tol, df0, nullptr, b_out, mu_out, h2_out, ve_out, vb_out, its_out, cnv_out, xb_out);
}

// solver2x (:1446-1493) for every column of Y: X1 = Z (dense, n x q), X2 = the panel
extern "C" int bwgr_uvbeta2(bwgr_panel *P, const double *Z, int64_t q, int64_t ldz, const double *Y, int64_t k, int maxit, double tol, double df0, double *b1_out,
                            double *b2_out, double *mu_out, double *h2_out, double *ve_out, double *vb1_out, double *vb2_out, int *its_out, double *cnv_out) {
  if (q < 1) return fail(BWGR_EINVAL, "uvbeta2: q = %lld columns of Z (at least 1)", (long long)q);
  if (!Z || !b1_out) return fail(BWGR_EINVAL, "uvbeta2: null pointer");
  UvDenseLeg D{Z, q, ldz, b1_out, vb1_out};
  return uvb_run("uvbeta2", P, Y, k, BWGR_UVB_D, maxit, tol, df0, &D, b2_out, mu_out, h2_out, ve_out, vb2_out, its_out, cnv_out, nullptr);
}


// ------------------------------------------------------------------------------------------------
// the same fits on a small dense design, and X B on the panel: the second stage and the products of XSEMF / ZSEMF / YSEMF
// (src/RcppEigen20230423.cpp:1756-1769, :1819-1874): the kernels of uvbd.hip.h
// ------------------------------------------------------------------------------------------------
extern "C" int bwgr_debug_uvbd_plan(int64_t n, int64_t q, int64_t k, int64_t out[BWGR_UVBD_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "uvbd plan: null pointer");
  if (n < 1 || q < 1 || k < 1) return fail(BWGR_EINVAL, "uvbd plan: n = %lld, q = %lld, k = %lld (each at least 1)", (long long)n, (long long)q, (long long)k);
  const UvbdPlan pl = uvbd_plan(n, q, k);
  out[0] = pl.lds_rows; out[1] = pl.e_in_lds ? 1 : 0; out[2] = pl.threads; out[3] = (int64_t)pl.lds_bytes; out[4] = (int64_t)pl.ws_bytes;
  return BWGR_OK;
}

extern "C" int bwgr_uvbeta_dense(int device, const double *Z, int64_t n, int64_t q, int64_t ldz, const double *Y, int64_t k, int variant, int maxit,
                                 double tol, double df0, double *b_out, double *mu_out, double *h2_out, double *ve_out, double *vb_out, int *its_out,
                                 double *cnv_out) {
  if (!Z || !Y || !b_out || !its_out) return fail(BWGR_EINVAL, "uvbeta_dense: null pointer");
  if (n < 1 || q < 1 || q > 0x7FFFFF00ll || ldz < n) return fail(BWGR_EINVAL, "uvbeta_dense: n = %lld rows, q = %lld columns, ldz = %lld (n, q at least 1, ldz at least n)", (long long)n, (long long)q, (long long)ldz);
  CHK(uvb_accept("uvbeta_dense", k, 0x7FFFFFFFll, variant, maxit));
  CHK(require_device(device));
  const UvbdPlan pl = uvbd_plan(n, q, k);
  const size_t nn = (size_t)n, nq = (size_t)q, nk = (size_t)k;
  // ---- host set-up: Z without its padding; Y on the traits' own rows, the masks as 0/1 bytes; every sweep's order ----
  std::vector<double> Zc;
  CHK(z_unpadded("uvbeta_dense", Z, n, q, ldz, Zc));
  TraitSet S;
  CHK(uvb_read("uvbeta_dense", Y, n, k, n, k, S));
  std::vector<UvbdTrait> tr(nk);
  for (size_t t = 0; t < nk; ++t) { tr[t].nt = S.nt[t]; tr[t].mu = S.mu[t]; tr[t].vy = S.vy[t]; }
  std::vector<int32_t> order(std::max<size_t>((size_t)maxit * nq, 1));
  CumulativeOrder ord(nq);
  for (int s = 0; s < maxit; ++s) {                                                                        // :1428 (cumulative, as there)
    const std::vector<int> &o = ord.next(s);
    std::copy(o.begin(), o.end(), order.begin() + (size_t)s * nq);
  }
  std::vector<double> res(nk * UVBD_NRES);
  hipStream_t st = nullptr;   // (the null stream: the holder waits for it before the vectors above go away)
  DevBufs bufs(st);
  double *Zd = bufs.get<double>(nn * nq), *yd = bufs.get<double>(nk * nn), *cols = bufs.get<double>(nk * 3 * nq), *bd = bufs.get<double>(nq * nk);
  double *resd = bufs.get<double>(nk * UVBD_NRES), *ews = pl.e_in_lds ? nullptr : bufs.get<double>(pl.ws_bytes / sizeof(double));
  uint8_t *md = bufs.get<uint8_t>(nk * nn);
  UvbdTrait *trd = bufs.get<UvbdTrait>(nk);
  int32_t *ordd = bufs.get<int32_t>(order.size());
  if (bufs.failed()) return no_memory("uvbeta_dense");
  HIPCHK(h2d(st, Zd, Zc.data(), Zc.size()));
  HIPCHK(h2d(st, yd, S.y.data(), S.y.size()));
  HIPCHK(h2d(st, md, S.obs.data(), S.obs.size()));
  HIPCHK(h2d(st, trd, tr.data(), tr.size()));
  HIPCHK(h2d(st, ordd, order.data(), order.size()));
  HIPCHK(zero(st, bd, nq * nk));                                                                           // b = 0, :1421
  UvbdArgs A;
  A.Z = Zd; A.n = n; A.q = q; A.y = yd; A.m = md; A.tr = trd; A.order = ordd; A.variant = variant; A.maxit = maxit;
  A.logtol = log10(tol); A.df0 = df0; A.thr = variant == BWGR_UVB_F ? 0.00001 : 0.0;
  A.cols = cols; A.e_ws = ews; A.b = bd; A.res = resd;
  if (pl.e_in_lds) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvbd_fit<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)UVBD_LDS_MAX));
    hipLaunchKernelGGL(k_uvbd_fit<true>, dim3((unsigned)k), dim3(pl.threads), pl.lds_bytes, st, A);
  } else {
    hipLaunchKernelGGL(k_uvbd_fit<false>, dim3((unsigned)k), dim3(pl.threads), pl.lds_bytes, st, A);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, b_out, bd, sizeof(double) * nq * nk));
  HIPCHK(d2h(st, res.data(), resd, sizeof(double) * nk * UVBD_NRES));
  const UvbOut out = {mu_out, h2_out, ve_out, vb_out, cnv_out, its_out};
  for (int64_t t = 0; t < k; ++t) {
    const double *rt = res.data() + (size_t)t * UVBD_NRES;
    uvb_result(out, t, S.nt[(size_t)t] == 0.0, variant, rt[0], rt[1], rt[2], S.vy[(size_t)t], rt[3], (int)rt[4]);
  }
  return BWGR_OK;
}

// out = X B on the raw int8 genotypes, every row: k_pxb over (row tiles, marker chunks, 16-trait slices), then the chunks' partials in order.
// The chunks: as many as bring the grid to about four workgroups per compute unit, at most 64 and never shorter than one staged tile of B.
static constexpr int PXB_CHUNKS_MAX = 64;     // marker chunks at most (before the chunk is rounded up to whole staged tiles of B)
static constexpr int PXB_FINISH_WG = 4096;    // workgroups of k_pxb_finish at most, 256 entries each per trip
static inline int64_t pxb_finish_grid(int64_t nk) { return std::min<int64_t>((nk + TAIL_THREADS - 1) / TAIL_THREADS, PXB_FINISH_WG); }
struct PxbPlan { int64_t tiles, slices, chunks, chunk; };
static PxbPlan pxb_plan(int64_t ld, int64_t p, int64_t k) {
  PxbPlan pl;
  pl.tiles = (ld + PXB_ROWS - 1) / PXB_ROWS; pl.slices = (k + PXB_TS - 1) / PXB_TS;
  pl.chunks = std::min<int64_t>(std::min<int64_t>(PXB_CHUNKS_MAX, (p + PXB_MT - 1) / PXB_MT), std::max<int64_t>(1, (1024 + pl.tiles * pl.slices - 1) / (pl.tiles * pl.slices)));
  pl.chunk = ((p + pl.chunks - 1) / pl.chunks + PXB_MT - 1) / PXB_MT * PXB_MT;
  pl.chunks = (p + pl.chunk - 1) / pl.chunk;
  return pl;
}
extern "C" int bwgr_panel_xb(bwgr_panel *P, const double *B, int64_t k, double *out) {
  if (!P || !B || !out) return fail(BWGR_EINVAL, "panel_xb: null pointer");
  if (k < 1 || k > 0x7FFFFFFFll) return fail(BWGR_EINVAL, "panel_xb: k = %lld columns (at least 1)", (long long)k);
  if (P->data->is_f32) return fail(BWGR_EINVAL, "panel_xb: the panel holds fp32 genotypes; panel_xb takes int8 panels only");
  HIPCHK(hipSetDevice(P->data->device));
  const int64_t n = P->data->n, p = P->data->p, ld = P->data->plan.ld;
  const int R = P->data->plan.R;
  const PxbPlan xp = pxb_plan(ld, p, k);
  const int64_t tiles = xp.tiles, slices = xp.slices, chunks = xp.chunks, chunk = xp.chunk;
  if (slices > 65535) return fail(BWGR_EINVAL, "panel_xb: k = %lld columns (at most %d per call)", (long long)k, 65535 * PXB_TS);
  hipStream_t st = P->stream;
  DevBufs bufs(st);
  const size_t nk = (size_t)n * (size_t)k;
  double *Bd = bufs.get<double>((size_t)p * (size_t)k), *part = bufs.get<double>((size_t)chunks * nk), *outd = bufs.get<double>(nk);
  if (bufs.failed()) return no_memory("panel_xb");
  HIPCHK(h2d(st, Bd, B, (size_t)p * (size_t)k));
  hipLaunchKernelGGL(k_pxb, dim3((unsigned)tiles, (unsigned)chunks, (unsigned)slices), dim3(256), 0, st, (const int8_t *)P->data->X, R, p, ld, n, (const double *)Bd, (int)k,
                     chunk, part);
  hipLaunchKernelGGL(k_pxb_finish, dim3((unsigned)pxb_finish_grid((int64_t)nk)), dim3(TAIL_THREADS), 0, st, (const double *)part, (int64_t)nk, (int)chunks, outd);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, out, outd, sizeof(double) * nk));
  return BWGR_OK;
}
