// bwgr_amd/csrc/kernels_host.hip.h -- the host entries of the relationship kernels: the exact X X' of an int8 panel, the exact X_f X_s'
// between two, and their fp64 finishes (kernels.hip.h).  Part of bwgr_hip.hip, after uvb_host.hip.h; it defines no kernel.
// ------------------------------------------------------------------------------------------------
// A product's plan, decided here and nowhere else (bwgr_debug_xxt_plan and bwgr_debug_xyt_plan expose it to the CPU tests): the chunk of
// markers whose int32 sums are exact for the panels' largest |x|, the tiles -- those on and above the diagonal of X X' (sym), every tile of
// the T_r x T_c grid of X_f X_s' -- and how far a chunk is split again so that small n still fills the chip; integer sums make every split
// give the same bits.
struct XxtPlan {
  bool sym = true;                  // X X' of one panel (rows = columns); or X_f X_s' between two
  int64_t chunk = 0, nchunks = 0;   // markers per int32 chunk (the rule's, or the forced one); chunks
  int64_t Tr = 0, Tc = 0, tiles = 0;   // row and column tiles of XXT_TILE rows; tiles computed
  int64_t sub = 1, piece = 0;       // pieces per chunk; markers per piece (whole MFMA steps)
  int64_t wgs = 0;                  // workgroups launched: tiles x chunks x pieces
  bool accumulate = false;          // more than one workgroup per tile: they add into the zeroed int64 tile
  size_t ws_bytes = 0;              // device temporaries of a kernel / kernel2 call with host outputs
};
static constexpr int XXT_SUMD_PARTS = 1024;
static constexpr int XXT_ZERO_WG = 2048;      // workgroups of k_xxt_zero, 256 entries each per trip
static constexpr int KFIN_APPLY_WG = 4096;    // workgroups of k_kfin_apply / k_kfin2_apply, 256 entries each per trip
// nr, xmaxr: the rows' panel (X; the founders); nc, xmaxc: the columns' (sym: the same panel again; the samples)
static int plan_xxt(XxtPlan &pl, bool sym, int64_t nr, int64_t nc, int64_t p, int xmaxr, int xmaxc, int64_t kchunk) {
  pl = XxtPlan();
  pl.sym = sym;
  const char *who = sym ? "xxt" : "xyt", *Xr = sym ? "X" : "X_f", *Xc = sym ? "X" : "X_s";
  CHK(panel_range(nr, p));
  CHK(panel_range(nc, p));
  if (xmaxr < 0 || xmaxr > 128 || xmaxc < 0 || xmaxc > 128) return fail(BWGR_EINVAL, "%s: largest |x| = %d, %d are not int8 panels'", who, xmaxr, xmaxc);
  if (kchunk < 0) return fail(BWGR_EINVAL, "%s: forced chunk %lld < 0", who, (long long)kchunk);
  const int64_t xr = std::max(xmaxr, 1), xc = std::max(xmaxc, 1), x2 = xr * xc;
  if ((long double)x2 * (long double)p >= 9007199254740992.0L)
    return fail(BWGR_EINVAL, "%s: max|x| of %s * max|x| of %s * p = %.3Lg reaches 2^53: the entries of %s %s' would not be exact doubles", who, Xr, Xc,
                (long double)x2 * (long double)p, Xr, Xc);
  // the bounds on X s: the column sums s are the rows' panel's, applied to either panel
  if ((long double)(xr * xr) * (long double)nr * (long double)p >= 9223372036854775808.0L)
    return fail(BWGR_EINVAL, "%s: max|x|^2 * n * p of %s = %.3Lg reaches 2^63: %s s would not fit int64", who, Xr, (long double)(xr * xr) * (long double)nr * (long double)p, Xr);
  if ((long double)x2 * (long double)nr * (long double)p >= 9223372036854775808.0L)
    return fail(BWGR_EINVAL, "%s: max|x| of %s * max|x| of %s * n * p = %.3Lg reaches 2^63: %s s would not fit int64", who, Xr, Xc,
                (long double)x2 * (long double)nr * (long double)p, Xc);
  const int64_t rule = 2147483647ll / x2;
  pl.chunk = kchunk > 0 ? std::min(kchunk, rule) : rule;   // (a forced chunk beyond the rule would not be exact)
  pl.nchunks = (p + pl.chunk - 1) / pl.chunk;
  pl.Tr = (nr + XXT_TILE - 1) / XXT_TILE; pl.Tc = (nc + XXT_TILE - 1) / XXT_TILE;
  pl.tiles = sym ? pl.Tr * (pl.Tr + 1) / 2 : pl.Tr * pl.Tc;
  // pieces: about four workgroups per compute unit where the tiles and chunks alone give fewer, never shorter than sixteen steps
  const int64_t span = std::min(pl.chunk, p), steps = (span + XXT_KSTEP - 1) / XXT_KSTEP;
  const int64_t want = (1024 + pl.tiles * pl.nchunks - 1) / (pl.tiles * pl.nchunks);
  const int64_t sub0 = std::max<int64_t>(1, std::min(want, steps / 16));
  pl.piece = (steps + sub0 - 1) / sub0 * XXT_KSTEP;
  pl.sub = (span + pl.piece - 1) / pl.piece;
  if (pl.nchunks * pl.sub > 65535) return fail(BWGR_EINVAL, "%s: %lld chunks of %lld markers exceed the launch grid (65535); use a longer BWGR_KCHUNK", who, (long long)pl.nchunks, (long long)pl.chunk);
  if (pl.tiles > 0x7FFFFFFFll) return fail(BWGR_EINVAL, "%s: %lld output tiles exceed the launch grid", who, (long long)pl.tiles);
  pl.wgs = pl.tiles * pl.nchunks * pl.sub;
  pl.accumulate = pl.nchunks * pl.sub > 1;
  const int64_t ldr = (nr + 127) / 128 * 128, ldc = (nc + 127) / 128 * 128;   // (at least; a panel's own padding may be larger)
  // kernel: the n x n array; s and q; X s; the diagonal; the partial sums
  if (sym) pl.ws_bytes = (size_t)nr * nr * 8 + (size_t)p * 12 + (size_t)ldr * 8 + (size_t)nr * 8 + (size_t)(XXT_SUMD_PARTS + 1) * 8;
  // kernel2: the two 8-byte arrays; s and q; X_f s, X_s s and the samples' row sums of squares; the founders' diagonal; the partial sums;
  // the two double terms per founder and per sample of the ARC finish
  else pl.ws_bytes = (size_t)nr * nc * 8 + (size_t)nr * nr * 8 + (size_t)p * 12 + (size_t)(ldr + 2 * ldc) * 8 + (size_t)nr * 8 + (size_t)(XXT_SUMD_PARTS + 1) * 8 +
                     (size_t)(nr + nc) * 16;
  return BWGR_OK;
}
extern "C" int bwgr_debug_xxt_plan(int64_t n, int64_t p, int xmax, int64_t kchunk, int64_t out[BWGR_XXT_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "debug_xxt_plan: null pointer");
  XxtPlan pl;
  CHK(plan_xxt(pl, true, n, n, p, xmax, xmax, kchunk));
  const int64_t v[BWGR_XXT_PLAN_NOUT] = {pl.chunk, pl.nchunks, pl.tiles, pl.wgs, (int64_t)pl.ws_bytes, pl.Tr, pl.sub, pl.piece};
  std::copy(v, v + BWGR_XXT_PLAN_NOUT, out);
  return BWGR_OK;
}
extern "C" int bwgr_debug_xyt_plan(int64_t nf, int64_t ns, int64_t p, int xmaxf, int xmaxs, int64_t kchunk, int64_t out[BWGR_XYT_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "debug_xyt_plan: null pointer");
  XxtPlan pl;
  CHK(plan_xxt(pl, false, nf, ns, p, xmaxf, xmaxs, kchunk));
  const int64_t v[BWGR_XYT_PLAN_NOUT] = {pl.chunk, pl.nchunks, pl.tiles, pl.wgs, (int64_t)pl.ws_bytes, pl.Tr, pl.Tc, pl.sub, pl.piece};
  std::copy(v, v + BWGR_XYT_PLAN_NOUT, out);
  return BWGR_OK;
}

// What every entry point checks of a panel it is given; `role` names the panel in the message ("", "founders' ", "samples' ").
static int kern_accept_panel(const bwgr_panel *P, int memloc, const char *who, const char *role) {
  if (!P) return fail(BWGR_EINVAL, "%s: null pointer", who);
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "%s: bad memloc %d", who, memloc);
  if (P->data->is_f32) return fail(BWGR_EINVAL, "%s: the %spanel holds fp32 genotypes; the relationship kernels take int8 panels only", who, role);
  return BWGR_OK;
}
// ... and the last check of a call, once its plan stands: these launches fill the chip, so nothing is enqueued while sweeps of other handles,
// whose workgroups must stay co-resident, are in flight (a pair: the partner's own work is waited for, xyt_order).  Leaves P's device set.
static int kern_accept_guard(bwgr_panel *P, const bwgr_panel *partner, const char *who) {
  HIPCHK(hipSetDevice(P->data->device));
  if (!P->data->sw.occ_guard) return BWGR_OK;
  std::lock_guard<std::mutex> lk(g_guard_mu);
  const int busy = guard_busy(P, P->stream, partner);
  if (busy > 0) return fail(BWGR_EINVAL, "%s: sweeps of other handles hold %d compute units on this device; wait for them (bwgr_chain_sync) and call again", who, busy);
  return BWGR_OK;
}
// what the two one-panel entry points check alike.  Nothing is enqueued before it returns BWGR_OK.
static int xxt_accept(bwgr_panel *P, const void *out, int64_t ldo, int memloc, const char *who, XxtPlan &pl) {
  if (!out) return fail(BWGR_EINVAL, "%s: null pointer", who);
  CHK(kern_accept_panel(P, memloc, who, ""));
  const PanelData *D = P->data;
  if (D->n < 2) return fail(BWGR_EINVAL, "%s: n = %lld (needs 2 rows)", who, (long long)D->n);
  if (ldo < D->n) return fail(BWGR_EINVAL, "%s: leading dimension %lld < n = %lld", who, (long long)ldo, (long long)D->n);
  CHK(plan_xxt(pl, true, D->n, D->n, D->p, D->xmax, D->xmax, D->sw.kchunk));
  return kern_accept_guard(P, nullptr, who);
}
// what the two two-panel entry points check alike.  Nothing is enqueued before it returns BWGR_OK.
static int xyt_accept(bwgr_panel *Pf, bwgr_panel *Ps, int memloc, const char *who, XxtPlan &pl) {
  CHK(kern_accept_panel(Pf, memloc, who, "founders' "));
  CHK(kern_accept_panel(Ps, memloc, who, "samples' "));
  const PanelData *F = Pf->data, *S = Ps->data;
  if (F->p != S->p) return fail(BWGR_EINVAL, "%s: the founders have p = %lld markers, the samples %lld", who, (long long)F->p, (long long)S->p);
  if (F->device != S->device) return fail(BWGR_EINVAL, "%s: the founders are on device %d, the samples on device %d", who, F->device, S->device);
  CHK(plan_xxt(pl, false, F->n, S->n, F->p, F->xmax, S->xmax, F->sw.kchunk));
  return kern_accept_guard(Pf, Ps, who);
}
// the founders' stream goes on after everything pending on the samples' stream
static int xyt_order(bwgr_panel *Pf, bwgr_panel *Ps, DevBufs &bufs, const char *who) {
  if (Ps->stream == Pf->stream) return BWGR_OK;
  hipEvent_t ev = nullptr;
  HIPCHK(hand_over(bufs, &ev, Pf->stream, Ps->stream));
  return BWGR_OK;
}
// The planned product into the device array Gd (int64, row stride ldg), enqueued on Pr's stream: G = X X' over Pr's n rows, both triangles
// (pl.sym; Pc = Pr), or G = X_f X_s' (n_f x n_s) between the founders Pr and the samples Pc.
static int xxt_product(bwgr_panel *Pr, bwgr_panel *Pc, const XxtPlan &pl, long long *Gd, int64_t ldg) {
  const PanelData *A = Pr->data, *B = Pc->data;
  hipStream_t st = Pr->stream;
  XxtArgs a;
  a.XA = (const int8_t *)A->X; a.XB = (const int8_t *)B->X; a.p = A->p; a.RA = A->plan.R; a.RB = B->plan.R; a.nA = (int)A->n; a.nB = (int)B->n;
  a.T = (int)(pl.sym ? pl.Tr : pl.Tc); a.chunk = pl.chunk; a.piece = pl.piece; a.sub = (int)pl.sub; a.accumulate = pl.accumulate ? 1 : 0; a.G = Gd; a.ldg = ldg;
  const dim3 grid((unsigned)pl.tiles, (unsigned)(pl.nchunks * pl.sub));
  if (pl.accumulate) hipLaunchKernelGGL(k_xxt_zero, dim3(XXT_ZERO_WG), dim3(TAIL_THREADS), 0, st, Gd, ldg, a.nA, a.nB, pl.sym ? 1 : 0);
  if (pl.sym) {
    hipLaunchKernelGGL(k_xxt_mfma_i8, grid, dim3(256), 0, st, a);
    const unsigned t32 = (unsigned)((A->n + 31) / 32);
    hipLaunchKernelGGL(k_xxt_mirror, dim3(t32, t32), dim3(32, 8), 0, st, Gd, ldg, a.nA);
  } else {
    hipLaunchKernelGGL(k_xyt_mfma_i8, grid, dim3(256), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}
// an nr x nc 8-byte result to the caller's host array
static int kern_to_host(hipStream_t st, void *dst, int64_t ldo, const void *src, int64_t nr, int64_t nc) {
  HIPCHK(hipMemcpy2DAsync(dst, (size_t)ldo * 8, src, (size_t)nc * 8, (size_t)nc * 8, (size_t)nr, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BWGR_OK;
}
// the grid of k_kfin_xs / k_kfin2_rowsq over a panel of ld padded rows: 128 rows per workgroup, the markers split so that the launch fills the chip
static inline dim3 kfin_rows_grid(int64_t ld, int64_t p, int64_t *cpw) {
  const int64_t ysplit = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(65535, (p + 511) / 512), 2048 / (ld / 128) + 1));
  *cpw = (p + ysplit - 1) / ysplit;
  return dim3((unsigned)(ld / 128), (unsigned)((p + *cpw - 1) / *cpw));
}
// c = sum_j (s_j / n)^2 on the host, in marker order from the exact column sums
static double kfin_mean_sq(const std::vector<int32_t> &s, double ninv) {
  double c = 0.0;
  for (size_t j = 0; j < s.size(); ++j) { const double m = (double)s[j] * ninv; c += m * m; }
  return c;
}
// EigenGAU's and EigenGauZ's t = phi (-n (n - 1)) / sum_{i != j} sqrt(G_ii + G_jj - 2 G_ij) (RcppEigen20230423.cpp:37, :1929): the fixed-grid,
// fixed-tree sum over the n x n product G (part: XXT_SUMD_PARTS + 1 doubles), and n (n - 1) formed in double (the reference's int product
// overflows beyond 46 340 rows)
static int kfin_gau_t(hipStream_t st, const long long *G, int64_t ldg, const long long *diag_d, int64_t n, double par, double *part, double *t) {
  double sumd = 0.0;
  hipLaunchKernelGGL(k_kfin_sumd_stage1, dim3(XXT_SUMD_PARTS), dim3(256), 0, st, G, ldg, diag_d, (int)n, part);
  hipLaunchKernelGGL(k_kfin_sumd_stage2, dim3(1), dim3(256), 0, st, part, XXT_SUMD_PARTS, part + XXT_SUMD_PARTS);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, &sumd, part + XXT_SUMD_PARTS, sizeof(double)));
  const double nd = (double)n;
  *t = par * (-(nd * (nd - 1.0))) / sumd;
  return BWGR_OK;
}

extern "C" int bwgr_panel_crossprod(bwgr_panel *P, int64_t *G, int64_t ldg, int memloc) {
  XxtPlan pl;
  CHK(xxt_accept(P, G, ldg, memloc, "panel_crossprod", pl));
  const int64_t n = P->data->n;
  DevBufs bufs(P->stream);
  long long *Gd = reinterpret_cast<long long *>(G); int64_t ldd = ldg;
  if (memloc == BWGR_HOST) {
    Gd = bufs.get<long long>((size_t)n * n); ldd = n;
    if (bufs.failed()) return no_memory("panel_crossprod");
  }
  CHK(xxt_product(P, P, pl, Gd, ldd));
  if (memloc == BWGR_HOST) return kern_to_host(P->stream, G, ldg, Gd, n, n);
  HIPCHK(hipStreamSynchronize(P->stream));
  return BWGR_OK;
}

extern "C" int bwgr_panel_kernel(bwgr_panel *P, int kind, double par, int flag, double *K, int64_t ldk, int memloc) {
  if (kind < BWGR_K_GRM || kind > BWGR_K_EIGEN_ARC) return fail(BWGR_EINVAL, "panel_kernel: unknown kind %d", kind);
  XxtPlan pl;
  CHK(xxt_accept(P, K, ldk, memloc, "panel_kernel", pl));
  const PanelData *D = P->data;
  const int64_t n = D->n, p = D->p, ld = D->plan.ld;
  hipStream_t st = P->stream;
  // which inputs the kind needs: the centred product (GRM; EigenGRM / EigenARC with their flag), the column sums (those, and GAU's mean)
  const bool cen = kind == BWGR_K_GRM || ((kind == BWGR_K_EIGEN_GRM || kind == BWGR_K_EIGEN_ARC) && flag != 0);
  const bool cols = cen || kind == BWGR_K_GAU;
  std::vector<long long> diag((size_t)n), rs, q;
  std::vector<int32_t> s;
  DevBufs bufs(st);
  long long *Gd = reinterpret_cast<long long *>(K); int64_t ldd = ldk;
  if (memloc == BWGR_HOST) { Gd = bufs.get<long long>((size_t)n * n); ldd = n; }
  long long *diag_d = bufs.get<long long>((size_t)n), *rs_d = cen ? bufs.get<long long>((size_t)ld) : nullptr, *q_d = cols ? bufs.get<long long>((size_t)p) : nullptr;
  int32_t *s_d = cols ? bufs.get<int32_t>((size_t)p) : nullptr;
  double *part = kind == BWGR_K_EIGEN_GAU ? bufs.get<double>(XXT_SUMD_PARTS + 1) : nullptr;
  if (bufs.failed()) return no_memory("panel_kernel");
  CHK(xxt_product(P, P, pl, Gd, ldd));
  hipLaunchKernelGGL(k_kfin_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Gd, ldd, (int)n, diag_d);
  if (cols) hipLaunchKernelGGL(k_kfin_colstats, dim3((unsigned)((p + 3) / 4)), dim3(256), 0, st, (const int8_t *)D->X, D->plan.R, (int)n, p, s_d, q_d);
  if (cen) {
    HIPCHK(zero(st, rs_d, (size_t)ld));
    int64_t cpw = 0;
    const dim3 g = kfin_rows_grid(ld, p, &cpw);
    hipLaunchKernelGGL(k_kfin_xs, g, dim3(256), 0, st, (const int8_t *)D->X, D->plan.R, p, s_d, cpw, rs_d);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(diag.data(), diag_d, sizeof(long long) * n, hipMemcpyDeviceToHost, st));
  if (cols) { s.resize((size_t)p); q.resize((size_t)p); HIPCHK(hipMemcpyAsync(s.data(), s_d, sizeof(int32_t) * p, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(q.data(), q_d, sizeof(long long) * p, hipMemcpyDeviceToHost, st)); }
  if (cen) { rs.resize((size_t)n); HIPCHK(hipMemcpyAsync(rs.data(), rs_d, sizeof(long long) * n, hipMemcpyDeviceToHost, st)); }
  HIPCHK(hipStreamSynchronize(st));
  // ---- the global scalars, on the host in a fixed order from the exact integers ----
  const double nd = (double)n, ninv = 1.0 / nd;
  const double c = kfin_mean_sq(s, ninv);   // sum_j mean_j^2 (s is empty where the kind needs no column sums)
  double sumvar = 0.0;               // sum_j fvar(x_j) = sum_j (q_j - s_j^2 / n) / (n - 1)
  __int128 ss = 0, tr = 0;           // sum_j s_j^2 = the sum of all entries of G; its trace
  for (int64_t j = 0; j < (cols ? p : 0); ++j) {
    sumvar += ((double)q[j] - (double)s[j] * (double)s[j] / nd) / (nd - 1.0);
    ss += (__int128)s[j] * s[j];
  }
  for (int64_t i = 0; i < n; ++i) tr += diag[i];
  const auto zz_diag = [&](int64_t i) { double v = (double)diag[i]; if (cen) v = v - ((double)rs[i] * ninv + (double)rs[i] * ninv) + c; return v; };
  KfinArgs a;
  a.G = Gd; a.ldg = ldd; a.n = (int)n; a.kind = kind; a.cen = cen ? 1 : 0; a.diag = diag_d; a.rs = rs_d; a.ninv = ninv; a.c = c; a.scale = 1.0;
  switch (kind) {
    case BWGR_K_GRM: a.scale = flag ? c / 2.0 : sumvar; break;                                          // Sum2pq, :1369-1373
    case BWGR_K_GAU: a.scale = (double)(2 * ((__int128)n * tr - ss)) / (nd * (nd - 1.0)); break;        // md, :1351-1353
    case BWGR_K_EIGEN_GRM: case BWGR_K_EIGEN_ARC: {
      double sd = 0.0;
      for (int64_t i = 0; i < n; ++i) sd += zz_diag(i) + (kind == BWGR_K_EIGEN_GRM ? 1.0 : 0.0);
      a.scale = 1.0 / (sd / nd);                                                                        // tmp, RcppEigen20230423.cpp:18, :50
    } break;
    default: CHK(kfin_gau_t(st, Gd, ldd, diag_d, n, par, part, &a.scale));                              // EigenGAU's tmp, :37
  }
  hipLaunchKernelGGL(k_kfin_apply, dim3(KFIN_APPLY_WG), dim3(TAIL_THREADS), 0, st, a);
  HIPCHK(hipGetLastError());
  if (memloc == BWGR_HOST) return kern_to_host(st, K, ldk, Gd, n, n);
  HIPCHK(hipStreamSynchronize(st));
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// founder-by-sample kernels: the two entries on a pair of int8 panels, EigenArcZ's / EigenGauZ's K_ff and K_fs (kernels.hip.h; DESIGN.md
// section 4.6)
// ------------------------------------------------------------------------------------------------
extern "C" int bwgr_panel_crossprod2(bwgr_panel *Pf, bwgr_panel *Ps, int64_t *G, int64_t ldg, int memloc) {
  if (!G) return fail(BWGR_EINVAL, "panel_crossprod2: null pointer");
  if (Pf && Ps && ldg < Ps->data->n) return fail(BWGR_EINVAL, "panel_crossprod2: leading dimension %lld < n_s = %lld", (long long)ldg, (long long)Ps->data->n);
  XxtPlan pl;
  CHK(xyt_accept(Pf, Ps, memloc, "panel_crossprod2", pl));
  const int64_t nf = Pf->data->n, ns = Ps->data->n;
  DevBufs bufs(Pf->stream);
  long long *Gd = reinterpret_cast<long long *>(G); int64_t ldd = ldg;
  if (memloc == BWGR_HOST) {
    Gd = bufs.get<long long>((size_t)nf * ns); ldd = ns;
    if (bufs.failed()) return no_memory("panel_crossprod2");
  }
  CHK(xyt_order(Pf, Ps, bufs, "panel_crossprod2"));
  CHK(xxt_product(Pf, Ps, pl, Gd, ldd));
  if (memloc == BWGR_HOST) return kern_to_host(Pf->stream, G, ldg, Gd, nf, ns);
  HIPCHK(hipStreamSynchronize(Pf->stream));
  return BWGR_OK;
}

extern "C" int bwgr_panel_kernel2(bwgr_panel *Pf, bwgr_panel *Ps, int kind, double par, double *Kff, int64_t ldff, double *Kfs, int64_t ldfs, int memloc) {
  if (kind != BWGR_KZ_ARC && kind != BWGR_KZ_GAU) return fail(BWGR_EINVAL, "panel_kernel2: unknown kind %d", kind);
  if (!Kff || !Kfs) return fail(BWGR_EINVAL, "panel_kernel2: null pointer");
  if (Pf && Ps && ldff < Pf->data->n) return fail(BWGR_EINVAL, "panel_kernel2: leading dimension %lld of Kff < n_f = %lld", (long long)ldff, (long long)Pf->data->n);
  if (Pf && Ps && ldfs < Ps->data->n) return fail(BWGR_EINVAL, "panel_kernel2: leading dimension %lld of Kfs < n_s = %lld", (long long)ldfs, (long long)Ps->data->n);
  XxtPlan pl;
  CHK(xyt_accept(Pf, Ps, memloc, "panel_kernel2", pl));
  const PanelData *F = Pf->data, *S = Ps->data;
  XxtPlan plf;      // K_ff's product is the symmetric one
  CHK(plan_xxt(plf, true, F->n, F->n, F->p, F->xmax, F->xmax, F->sw.kchunk));
  const int64_t nf = F->n, ns = S->n, p = F->p, ldf = F->plan.ld, lds = S->plan.ld;
  const bool arc = kind == BWGR_KZ_ARC;
  hipStream_t st = Pf->stream;
  std::vector<long long> diag((size_t)nf), qs, rf, rs;
  std::vector<int32_t> s;
  std::vector<double> h_r, h_d;     // ARC: r_f | r_s; d_f | d_s
  DevBufs bufs(st);
  long long *Gff = reinterpret_cast<long long *>(Kff), *Gfs = reinterpret_cast<long long *>(Kfs); int64_t ldd_ff = ldff, ldd_fs = ldfs;
  if (memloc == BWGR_HOST) { Gff = bufs.get<long long>((size_t)nf * nf); ldd_ff = nf; Gfs = bufs.get<long long>((size_t)nf * ns); ldd_fs = ns; }
  long long *diag_d = bufs.get<long long>((size_t)nf), *qs_d = bufs.get<long long>((size_t)lds);
  long long *rf_d = arc ? bufs.get<long long>((size_t)ldf) : nullptr, *rs_d = arc ? bufs.get<long long>((size_t)lds) : nullptr, *q_d = arc ? bufs.get<long long>((size_t)p) : nullptr;
  int32_t *s_d = arc ? bufs.get<int32_t>((size_t)p) : nullptr;
  double *r_d = arc ? bufs.get<double>((size_t)(nf + ns)) : nullptr, *d_d = arc ? bufs.get<double>((size_t)(nf + ns)) : nullptr;
  double *part = arc ? nullptr : bufs.get<double>(XXT_SUMD_PARTS + 1);
  if (bufs.failed()) return no_memory("panel_kernel2");
  CHK(xyt_order(Pf, Ps, bufs, "panel_kernel2"));
  CHK(xxt_product(Pf, Pf, plf, Gff, ldd_ff));
  CHK(xxt_product(Pf, Ps, pl, Gfs, ldd_fs));
  hipLaunchKernelGGL(k_kfin_diag, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, Gff, ldd_ff, (int)nf, diag_d);
  int64_t cpw = 0;
  HIPCHK(zero(st, qs_d, (size_t)lds));
  { const dim3 g = kfin_rows_grid(lds, p, &cpw); hipLaunchKernelGGL(k_kfin2_rowsq, g, dim3(256), 0, st, (const int8_t *)S->X, S->plan.R, p, cpw, qs_d); }
  if (arc) {
    hipLaunchKernelGGL(k_kfin_colstats, dim3((unsigned)((p + 3) / 4)), dim3(256), 0, st, (const int8_t *)F->X, F->plan.R, (int)nf, p, s_d, q_d);
    HIPCHK(zero(st, rf_d, (size_t)ldf)); HIPCHK(zero(st, rs_d, (size_t)lds));
    { const dim3 g = kfin_rows_grid(ldf, p, &cpw); hipLaunchKernelGGL(k_kfin_xs, g, dim3(256), 0, st, (const int8_t *)F->X, F->plan.R, p, s_d, cpw, rf_d); }
    { const dim3 g = kfin_rows_grid(lds, p, &cpw); hipLaunchKernelGGL(k_kfin_xs, g, dim3(256), 0, st, (const int8_t *)S->X, S->plan.R, p, s_d, cpw, rs_d); }
  }
  HIPCHK(hipGetLastError());
  Kfin2Args a;
  a.kind = arc ? KFIN2_ARC : KFIN2_GAU; a.irow = diag_d; a.icol = diag_d; a.rrow = a.rcol = a.drow = a.dcol = nullptr; a.c = 0.0; a.scale = 1.0;
  const double nd = (double)nf, ninv = 1.0 / nd;
  if (arc) {
    qs.resize((size_t)ns); rf.resize((size_t)nf); rs.resize((size_t)ns); s.resize((size_t)p);
    HIPCHK(hipMemcpyAsync(diag.data(), diag_d, sizeof(long long) * nf, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(qs.data(), qs_d, sizeof(long long) * ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rf.data(), rf_d, sizeof(long long) * nf, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rs.data(), rs_d, sizeof(long long) * ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s.data(), s_d, sizeof(int32_t) * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // ---- the global scalars and the per-row terms, on the host in a fixed order from the exact integers ----
    const double c = kfin_mean_sq(s, ninv);
    h_r.resize((size_t)(nf + ns)); h_d.resize((size_t)(nf + ns));
    for (int64_t i = 0; i < nf; ++i) { const double r = (double)rf[i] * ninv; h_r[i] = r; h_d[i] = (double)diag[i] - (r + r) + c; }
    for (int64_t j = 0; j < ns; ++j) { const double r = (double)rs[j] * ninv; h_r[nf + j] = r; h_d[nf + j] = (double)qs[j] - (r + r) + c; }
    double sd = 0.0;                   // the finished diagonal of K_ff before Kscalar: it depends on d_f alone
    for (int64_t i = 0; i < nf; ++i) sd += kfin2_arc(h_d[i], h_d[i], h_d[i]);
    a.c = c; a.scale = 1.0 / (sd / nd);                                                                 // Kscalar, RcppEigen20230423.cpp:1896
    HIPCHK(h2d(st, r_d, h_r.data(), (size_t)(nf + ns))); HIPCHK(h2d(st, d_d, h_d.data(), (size_t)(nf + ns)));
    a.rrow = r_d; a.drow = d_d;
  } else {
    CHK(kfin_gau_t(st, Gff, ldd_ff, diag_d, nf, par, part, &a.scale));                                  // tmp, :1929
  }
  // K_ff, then K_fs (both read the founders' diagonal, which K_ff's finish overwrites only in G: diag_d is the copy)
  a.G = Gff; a.ldg = ldd_ff; a.nr = (int)nf; a.nc = (int)nf; a.same = 1;
  if (arc) { a.rcol = r_d; a.dcol = d_d; }
  hipLaunchKernelGGL(k_kfin2_apply, dim3(KFIN_APPLY_WG), dim3(TAIL_THREADS), 0, st, a);
  a.G = Gfs; a.ldg = ldd_fs; a.nc = (int)ns; a.same = 0; a.icol = qs_d;
  if (arc) { a.rcol = r_d + nf; a.dcol = d_d + nf; }
  hipLaunchKernelGGL(k_kfin2_apply, dim3(KFIN_APPLY_WG), dim3(TAIL_THREADS), 0, st, a);
  HIPCHK(hipGetLastError());
  if (memloc == BWGR_HOST) { CHK(kern_to_host(st, Kff, ldff, Gff, nf, nf)); return kern_to_host(st, Kfs, ldfs, Gfs, nf, ns); }
  HIPCHK(hipStreamSynchronize(st));
  return BWGR_OK;
}
