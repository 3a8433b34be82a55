// bwgr_amd/csrc/panel_host.hip.h -- the resident panel on the host: the upload, the sweep scratch, the column statistics, the Gram builders and
// k_sweep3's share of the data (sweep3_build), panel_alloc / bwgr_panel_create / _clone / _destroy / _info / _stats / _set_stream, the scratch
// panels of KMUP2, wgr and bwgr_em, and what the families' entries share beside the sweep: the row gather, bwgr_debug_last_redo, the two-stage X * coef
// (bwgr_debug_aux_plan exposes both launch rules), bwgr_panel_set_centred / _centred.  Part of bwgr_hip.hip, which includes it after the handle
// structs and sweep_host.hip.h (guard_forget); the plans it executes are panel_plan.hip.h's.  It defines no kernel: those are panel.hip.h's.
// the words the workgroups poll (flags, delta granules, q words and the feeders' sums) live in one allocation
static int alloc_exchange(bwgr_panel *P) {
  const size_t K = (size_t)P->data->plan.K;
  const size_t fb = (sizeof(uint32_t) * (K + 1) * SW_FLAG_STRIDE + 255) & ~(size_t)255;
  const size_t gb = (sizeof(unsigned long long) * S2_NSLOT * SW_MAXM + 255) & ~(size_t)255;
  const size_t qb = sizeof(double) * S2_NSLOT * (K + 1) * SW_MAXM;
  P->xchg_bytes = fb + gb + qb;
  CHK(own_array(P->own, P->xchg, P->xchg_bytes, "panel scratch"));
  P->xflags = reinterpret_cast<uint32_t *>(P->xchg);
  P->dgran = reinterpret_cast<unsigned long long *>(P->xchg + fb);
  P->qpart = reinterpret_cast<double *>(P->xchg + fb + gb);
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// panel
// ------------------------------------------------------------------------------------------------
template <typename ST, typename XT>
static int upload(bwgr_panel *P, const void *X, int memloc, int64_t ldx) {
  const int64_t n = P->data->n, p = P->data->p;
  XT *dst = reinterpret_cast<XT *>(P->data->X);
  if (memloc == BWGR_DEVICE) {
    hipLaunchKernelGGL((k_convert<ST, XT>), dim3(4096), dim3(256), 0, P->stream, reinterpret_cast<const ST *>(X), ldx, dst, P->data->plan.ld, (int)n, (int64_t)0, p, P->data->plan.R, p);
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // host source: stage column chunks of <= 256 MiB
  const int64_t col_bytes = ldx * (int64_t)sizeof(ST);
  int64_t cols = std::max<int64_t>(1, ((int64_t)256 << 20) / std::max<int64_t>(1, col_bytes));
  cols = std::min(cols, p);
  DevBufs bufs;
  ST *stage = bufs.get<ST>((size_t)(cols * ldx));
  if (!stage) return fail(BWGR_ENOMEM, "panel_create: device allocation failed");
  for (int64_t j0 = 0; j0 < p; j0 += cols) {
    const int64_t nc = std::min(cols, p - j0);
    // the last column may be shorter than ldx in the caller's allocation: copy n rows of it separately
    const size_t bytes = (size_t)((nc - 1) * col_bytes + n * (int64_t)sizeof(ST));
    HIPCHK(hipMemcpyAsync(stage, reinterpret_cast<const ST *>(X) + j0 * ldx, bytes, hipMemcpyHostToDevice, P->stream));
    hipLaunchKernelGGL((k_convert<ST, XT>), dim3(2048), dim3(256), 0, P->stream, stage, ldx, dst, P->data->plan.ld, (int)n, j0, nc, P->data->plan.R, p);
    HIPCHK(hipStreamSynchronize(P->stream));
  }
  return BWGR_OK;
}

// A handle's sweep scratch, made once its data is built (the root's by whoever makes the data, a clone's by bwgr_panel_clone): the
// speculative cross terms of the distances whose Gram blocks the data has, the pre-staged constants, the exchange words, and k_sweep3's
// sums and lists where the data has k_sweep3.  The rest of the scratch comes with the first sweep that needs it; the handle's holder owns all of it.
static int scratch_alloc(bwgr_panel *P) {
  const PanelData *D = P->data;
  const size_t nb = (size_t)D->plan.nblocks;
  const char *who = "panel scratch";
  if (D->plan.xdist >= 2) CHK(own_array(P->own, P->xspec2, nb * SW_MAXM, who));
  if (D->plan.xdist >= 3) CHK(own_array(P->own, P->xspec3, nb * SW_MAXM, who));
  if (D->plan.pipelined) CHK(own_array(P->own, P->ps.quick, nb, who));
  if (!P->own.take({{&P->ps.spec, sizeof(SpecBuf) * nb}, {&P->ps.blocks, sizeof(StageBuf) * nb}, {&P->xpart, sizeof(double) * 2 * (size_t)D->plan.K * SW_MAXM}})) return no_memory(who);
  CHK(alloc_exchange(P));
#if defined(BWGR_STAMPS) || defined(BWGR_EXPERIMENTS)
  CHK(own_array(P->own, P->stamps, 256, who));
  HIPCHK(hipMemset(P->stamps, 0, sizeof(unsigned long long) * 256));
#endif
  if (D->e3_ready) {
    if (!P->own.take({{&P->qsum3, sizeof(unsigned long long) * 2 * SW_MAXM * nb}, {&P->lists3, sizeof(unsigned long long) * S3_LSTRIDE * nb}})) return no_memory(who);
    HIPCHK(hipMemsetAsync(P->lists3, 0, sizeof(unsigned long long) * S3_LSTRIDE * nb, P->stream));
  }
  return BWGR_OK;
}

extern "C" int bwgr_panel_destroy(bwgr_panel *P) {
  if (!P) return BWGR_OK;
  PanelData *D = P->data;
  if (P->is_root && D->nclones > 0) return fail(BWGR_EINVAL, "panel_destroy: %d clone(s) of this panel are still alive", D->nclones);
  if (P->nchains > 0) return fail(BWGR_EINVAL, "panel_destroy: %d chain(s) on this panel are still alive (destroy them first)", P->nchains);
  (void)hipSetDevice(D->device);
  guard_forget(P);
  if (P->pre_pair_set) pair_stream_count(D, P->stream, -1);
  const bool root = P->is_root;
  delete P;   // the handle's scratch and streams, then the data's arrays and the pair streams
  if (root) delete D;
  else D->nclones--;
  return BWGR_OK;
}

// a10's xx, vx and MSx, and an int8 panel's largest |x|
static int panel_measure(bwgr_panel *P) {
  PanelData *D = P->data;
  const int p = (int)D->p, n = (int)D->n, wpb = 4;
  if (D->is_f32) hipLaunchKernelGGL(k_stats<float>, dim3((p + wpb - 1) / wpb), dim3(64 * wpb), 0, P->stream, (const float *)D->X, D->plan.R, n, p, D->xx, D->vx);
  else hipLaunchKernelGGL(k_stats<int8_t>, dim3((p + wpb - 1) / wpb), dim3(64 * wpb), 0, P->stream, (const int8_t *)D->X, D->plan.R, n, p, D->xx, D->vx);
  HIPCHK(hipGetLastError());
  CHK(sum_floats(P->stream, {{D->vx, (int64_t)p, &D->MSx}}, "panel_create"));
  if (!D->is_f32) {
    if (!D->xmax_dev) CHK(own_array(D->own, D->xmax_dev, 1, "panel_create"));
    HIPCHK(hipMemsetAsync(D->xmax_dev, 0, sizeof(int), P->stream));
    hipLaunchKernelGGL(k_absmax_i8, dim3(2048), dim3(256), 0, P->stream, (const int8_t *)D->X, D->plan.x_bytes, D->xmax_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&D->xmax, D->xmax_dev, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
  }
  return BWGR_OK;
}

// f(std::integral_constant<int, TJ>()) with TJ = tj, 1 <= tj <= MAXTJ (beyond: MAXTJ): the Gram kernels' block width in sixteens as a template parameter
template <int MAXTJ, typename F> static void with_tj(int tj, F f) {
  if constexpr (MAXTJ > 1) { if (tj < MAXTJ) return with_tj<MAXTJ - 1>(tj, f); }
  f(std::integral_constant<int, MAXTJ>());
}
// Gram blocks X_{b-dist}' X_b of the resident X, b = dist .. nblocks-1, into g[b][m][m]: int32, exact (fp64 for float panels); dist = 0: the diagonal blocks
static void launch_gram(bwgr_panel *P, void *g, int dist) {
  const PanelPlan &pl = P->data->plan;
  const int p = (int)P->data->p, m = pl.m, R = pl.R, tiles = dist ? 2 : 1;
  const dim3 grid((unsigned)(pl.nblocks - dist)), block(256);
  const int64_t ld = pl.ld; hipStream_t st = P->stream;
  const size_t ldsf = (size_t)tiles * m * 65 * sizeof(float), ldsi = (size_t)tiles * m * 33 * sizeof(int32_t);   // the kernels' LDS tiles
  const float *Xf = (const float *)P->data->X; double *gd = (double *)g;
  const int8_t *Xi = (const int8_t *)P->data->X; int32_t *gi = (int32_t *)g;
  const bool f32 = P->data->is_f32 != 0;
  if (!f32 && m == 128) hipLaunchKernelGGL(k_gram_mfma_i8, grid, block, 0, st, Xi, ld, R, p, gi, dist);
  else if (!f32 && dist) with_tj<8>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gramx_i8<decltype(tj)::value>, grid, block, ldsi, st, Xi, ld, R, p, m, gi, dist); });
  else if (f32 && !dist) with_tj<4>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gram_f32<decltype(tj)::value>, grid, block, ldsf, st, Xf, ld, R, p, m, gd); });
  else if (!dist) with_tj<8>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gram_i8<decltype(tj)::value>, grid, block, ldsi, st, Xi, ld, R, p, m, gi); });
  else with_tj<4>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gramx_f32<decltype(tj)::value>, grid, block, ldsf, st, Xf, ld, R, p, m, gd, dist); });
}

// the Gram kernels sum a column pair of an int8 panel over every row in int32 (include/bwgr.h, at bwgr_panel_create)
static int gram_range(bool is_f32, int64_t rows, int xmax) {
  const int64_t xm = std::max(xmax, 1);
  if (!is_f32 && rows * xm * xm >= (1ll << 31)) return fail(BWGR_EINVAL, "panel: n * max|x|^2 = %lld does not fit the int32 Gram", (long long)(rows * xm * xm));
  return BWGR_OK;
}
// The Gram arrays the plan lists, from the resident X, and what they say: whether the 16-bit copies are exact (gram16) and how far the affine
// engine's byte planes reach (winv_nd).  Runs again wherever a scratch panel's rows or columns change.
static int panel_build_gram(bwgr_panel *P) {
  PanelData *D = P->data; const PanelPlan &pl = D->plan;
  const int m = pl.m;
  CHK(gram_range(D->is_f32 != 0, D->n, D->xmax));   // (a main panel's largest |x| is known only now; a scratch panel was checked before it was allocated)
  launch_gram(P, D->gram, 0);
  HIPCHK(hipGetLastError());
  for (int dist = 1; dist <= pl.xdist && dist < pl.nblocks; ++dist) {   // off-diagonal blocks (blk-dist, blk): the cross terms of the lag-2 / 3 / 4 pipelines
    launch_gram(P, D->gx[dist], dist);
    HIPCHK(hipGetLastError());
  }
  if (D->is_f32) hipLaunchKernelGGL(k_gram_pack<double>, dim3((unsigned)pl.nblocks), dim3(256), 0, P->stream, (const double *)D->gram, (double *)D->gramp, m, pl.pstride, pl.nblocks);
  else hipLaunchKernelGGL(k_gram_pack<int32_t>, dim3((unsigned)pl.nblocks), dim3(256), 0, P->stream, (const int32_t *)D->gram, (int32_t *)D->gramp, m, pl.pstride, pl.nblocks);
  HIPCHK(hipGetLastError());
  D->gram16 = false;
  if (pl.has16) {
    HIPCHK(hipMemsetAsync(D->gram16_bad, 0, sizeof(int), P->stream));
    hipLaunchKernelGGL(k_gram_narrow, dim3(2048), dim3(256), 0, P->stream, (const int32_t *)D->gramp, D->gramp16, (int64_t)pl.nblocks * pl.pstride, D->gram16_bad);
    if (pl.nblocks > 1)
      hipLaunchKernelGGL(k_gram_narrow, dim3(2048), dim3(256), 0, P->stream, (const int32_t *)D->gx[1] + (size_t)m * m, D->gramx16 + (size_t)m * m, (int64_t)(pl.nblocks - 1) * m * m, D->gram16_bad);
    HIPCHK(hipGetLastError());
    int bad = 1;
    HIPCHK(hipMemcpyAsync(&bad, D->gram16_bad, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
    D->gram16 = (bad == 0) && D->sw.gram16;   // BWGR_GRAM16=0 forces the 32-bit staging (A/B tests)
  }
  // the affine sweeps' sequencer (sweep2w.hip.h) takes the cross blocks as biased byte planes: built where every entry fits 16 bits
  D->winv_nd = 0;
  if (D->gram16 && pl.wdist > 0) {
    HIPCHK(hipMemsetAsync(D->gram16_bad, 0, sizeof(int), P->stream));
    int nd = 0;
    DevBufs bufs;
    int32_t *tmpx = nullptr;   // the distances beyond the panel's own arrays: built here, kept as planes only
    for (int dist = 1; dist <= pl.wdist; ++dist) {
      if (dist > S2W_NEARD) {
        if (!tmpx && !(tmpx = bufs.get<int32_t>((size_t)pl.nblocks * m * m))) { (void)hipGetLastError(); break; }
        launch_gram(P, tmpx, dist);
      }
      const int32_t *src = dist > S2W_NEARD ? tmpx : (const int32_t *)D->gx[dist];
      if (!D->gxt[dist - 1]) CHK(own_array(D->own, D->gxt[dist - 1], (size_t)pl.nblocks * S2W_PBYTES, "panel_create"));
      hipLaunchKernelGGL(k_gx_planes, dim3(4096), dim3(256), 0, P->stream, src, D->gxt[dist - 1], m, (int64_t)pl.nblocks, dist, D->gram16_bad);
      HIPCHK(hipGetLastError());
      nd = dist;
    }
    int bad = 1;
    HIPCHK(hipMemcpyAsync(&bad, D->gram16_bad, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
    D->winv_nd = bad ? 0 : nd;
  }
  HIPCHK(hipStreamSynchronize(P->stream));
  return BWGR_OK;
}

// ---- k_sweep3 (sweep3.hip.h): what it needs beside the panel ----
// plan3, then the cross Gram arrays of distance 1 .. D-1 in the element type of the 16-bit (or, failing that, 32-bit) staging
static int sweep3_build(bwgr_panel *P) {
  PanelData *D = P->data; const PanelPlan &pl = D->plan;
  D->e3_ready = false;
  D->plan3 = plan_panel3(pl, D->sw, D->gram16);
  if (!D->plan3.fits) return BWGR_OK;
  const int m = pl.m; const bool g16 = D->gram16;
  const size_t blk_elems = (size_t)pl.nblocks * m * m;
  int bad = 0;
  std::vector<void *> far;   // the arrays made here
  {   // the far blocks; tmp, a whole Gram array, goes once they are built and before the 16-bit verdict is acted on
    DevBufs bufs;
    int32_t *tmp = nullptr;
    for (int d = 1; d < D->plan3.D && d < pl.nblocks; ++d) {
      void *have32 = d <= pl.xdist ? D->gx[d] : nullptr, *have = g16 ? (d == 1 ? (void *)D->gramx16 : nullptr) : have32;
      if (have) { D->g3x[d - 1] = have; continue; }
      void *arr = nullptr;
      CHK(own_array(D->own, arr, blk_elems * (g16 ? 2 : 4), "panel_create"));
      D->g3x[d - 1] = arr; far.push_back(arr);
      if (g16) {
        if (!have32) {
          if (!tmp && !(tmp = bufs.get<int32_t>(blk_elems))) return fail(BWGR_ENOMEM, "panel_create: device allocation failed");
          launch_gram(P, tmp, d);
          have32 = tmp;
        }
        hipLaunchKernelGGL(k_gram_narrow, dim3(2048), dim3(256), 0, P->stream, (const int32_t *)have32 + (size_t)d * m * m, (uint16_t *)arr + (size_t)d * m * m, (int64_t)(pl.nblocks - d) * m * m, D->gram16_bad);
      } else launch_gram(P, arr, d);
      HIPCHK(hipGetLastError());
    }
    if (g16) HIPCHK(hipMemcpyAsync(&bad, D->gram16_bad, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
  }
  if (bad) {   // an entry of a far block left the 16-bit range although the near blocks fit: rare; leave the panel to k_sweep2
    for (void *q : far) D->own.drop(q);
    for (void *&g : D->g3x) g = nullptr;
    return BWGR_OK;
  }
  if (g16) {   // 16-bit panels: an included marker's distance-1 / 2 rows in one piece
    CHK(own_array(D->own, D->gx12, (size_t)pl.nblocks * m * 2 * m * 2, "panel_create"));
    hipLaunchKernelGGL(k_near_rows, dim3(4096), dim3(256), 0, P->stream, (const uint16_t *)D->g3x[0], (const uint16_t *)(D->plan3.D >= 3 ? D->g3x[1] : nullptr), (uint16_t *)D->gx12, m, (int64_t)pl.nblocks);
    HIPCHK(hipGetLastError());
  }
  for (const void *f : {reinterpret_cast<const void *>(k_sweep3<uint16_t, false>), reinterpret_cast<const void *>(k_sweep3<int32_t, false>), reinterpret_cast<const void *>(k_sweep3<uint16_t, true>),
                        reinterpret_cast<const void *>(k_sweep3<int32_t, true>), reinterpret_cast<const void *>(k_sweep3p<uint16_t>), reinterpret_cast<const void *>(k_sweep3p<int32_t>),
                        reinterpret_cast<const void *>(k_sweep3f)})
    HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  D->e3_ready = true;
  return BWGR_OK;
}

// what only the data can say, each from the last: the columns' statistics, the Gram arrays and their verdicts, k_sweep3's share where the plan tries it
static int panel_setup(bwgr_panel *P) {
  CHK(panel_measure(P));
  CHK(panel_build_gram(P));
  return sweep3_build(P);
}

// The data of a panel of n rows x p markers -- its plan and every device array the plan lists, no values yet -- and its root handle, without
// the sweep scratch (scratch_alloc, once the data is built)
static int panel_alloc(bwgr_panel **out, int is_f32, int64_t n, int64_t p, int device, int block, int nwg, PanelKind kind, const Switches &sw) {
  *out = nullptr;
  CHK(panel_range(n, p));
  CHK(require_device(device));
  PanelPlan pl;
  CHK(plan_panel(pl, is_f32 != 0, n, p, block, nwg, kind, sw));
  bwgr_panel *P = new bwgr_panel();
  PanelData *D = P->data = new PanelData(); P->is_root = true;
  Guard drop([&] { bwgr_panel_destroy(P); });   // until the panel is handed over
  D->device = device; D->n = n; D->p = p; D->is_f32 = is_f32; D->sw = sw; D->plan = pl;
  const size_t packed = (size_t)pl.nblocks * std::max(pl.pstride, 8);
  if (!D->own.take({{&D->X, pl.x_bytes}, {&D->gram, pl.gram_bytes}, {&D->gramp, packed * (is_f32 ? 8 : 4)}, {&D->xx, sizeof(float) * p}, {&D->vx, sizeof(float) * p}}))
    return no_memory("panel_create");
  for (int d = 1; d <= pl.xdist; ++d) CHK(own_array(D->own, D->gx[d], pl.gram_bytes, "panel_create"));
  if (pl.has16 && !D->own.take({{&D->gramp16, packed * 2}, {&D->gramx16, (size_t)pl.nblocks * pl.m * pl.m * 2}, {&D->gram16_bad, sizeof(int)}})) return no_memory("panel_create");
  for (const void *f : {reinterpret_cast<const void *>(k_sweep<int8_t, true>), reinterpret_cast<const void *>(k_sweep<int8_t, false>), reinterpret_cast<const void *>(k_sweep<float, true>),
                        reinterpret_cast<const void *>(k_sweep<float, false>), reinterpret_cast<const void *>(k_sweep2<int8_t, true>), reinterpret_cast<const void *>(k_sweep2<int8_t, false>),
                        reinterpret_cast<const void *>(k_sweep2<int8_t, true, uint16_t>), reinterpret_cast<const void *>(k_sweep2<float, true>), reinterpret_cast<const void *>(k_sweep2<float, false>),
                        reinterpret_cast<const void *>(k_sweep2w<true>), reinterpret_cast<const void *>(k_sweep2w<false>), reinterpret_cast<const void *>(k_affine_inv)})
    HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  drop.release();
  *out = P;
  return BWGR_OK;
}
// A scratch panel of P on P's stream: `rows` rows of P's markers (KMUP2, wgr's bagging) or P's columns in another order (bwgr_em).  Either's largest
// |x| is at most P's, so the scratch panel carries P's: panel_build_gram's int32 bound and the fixed-point scales of its sweeps (launch_prestage) are
// then those of the main panel, without a pass over the data.
static int scratch_panel_alloc(bwgr_panel **out, const bwgr_panel *P, int64_t rows, int nwg, PanelKind kind) {
  const PanelData *D = P->data;
  *out = nullptr;
  CHK(gram_range(D->is_f32 != 0, rows, D->xmax));   // refused before anything is allocated or enqueued
  CHK(panel_alloc(out, D->is_f32, rows, D->p, D->device, D->plan.m, nwg, kind, D->sw));
  (*out)->stream = P->stream;
  (*out)->data->xmax = D->xmax;
  return BWGR_OK;
}

extern "C" int bwgr_panel_create(bwgr_panel **out, const void *X, int xtype, int memloc, int64_t n, int64_t p,
                                 int64_t ldx, int device, int block, int nwg) {
  if (!out || !X) return fail(BWGR_EINVAL, "panel_create: null pointer");
  *out = nullptr;
  if (ldx < n) return fail(BWGR_EINVAL, "panel_create: need ldx >= n (n=%lld ldx=%lld)", (long long)n, (long long)ldx);
  if (xtype != BWGR_X_I8 && xtype != BWGR_X_F32 && xtype != BWGR_X_F64) return fail(BWGR_EINVAL, "panel_create: bad xtype %d", xtype);
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "panel_create: bad memloc %d", memloc);
  bwgr_panel *P = nullptr;
  CHK(panel_alloc(&P, xtype != BWGR_X_I8, n, p, device, block, nwg, PANEL_MAIN, read_switches()));
  Guard drop([&] { bwgr_panel_destroy(P); });
  if (xtype == BWGR_X_I8) CHK((upload<int8_t, int8_t>(P, X, memloc, ldx)));
  else if (xtype == BWGR_X_F32) CHK((upload<float, float>(P, X, memloc, ldx)));
  else CHK((upload<double, float>(P, X, memloc, ldx)));
  CHK(panel_setup(P));
  CHK(scratch_alloc(P));
  HIPCHK(hipStreamSynchronize(P->stream));   // handed over with nothing pending (k_sweep3's lists are zeroed on it): whoever gives the handle another stream orders nothing
  drop.release();
  *out = P;
  return BWGR_OK;
}

#if defined(BWGR_STAMPS) || defined(BWGR_EXPERIMENTS)
// diagnostic builds only: cumulative per-phase s_memtime ticks of workgroup 0, event counters (not part of include/bwgr.h)
extern "C" int bwgr_debug_stamps(bwgr_panel *P, unsigned long long out[256]) {
  HIPCHK(d2h(P->stream, out, P->stamps, sizeof(unsigned long long) * 256));
  HIPCHK(hipMemset(P->stamps, 0, sizeof(unsigned long long) * 256));
  return BWGR_OK;
}
#endif

// A clone: a second handle on the same data (the genotypes and Gram arrays are read-only during sweeps) with its own sweep scratch and its
// own stream, so that chains on the root panel and on its clones run concurrently on disjoint CUs.
extern "C" int bwgr_panel_clone(bwgr_panel **out, bwgr_panel *src) {
  if (!out || !src) return fail(BWGR_EINVAL, "panel_clone: null pointer");
  *out = nullptr;
  HIPCHK(hipSetDevice(src->data->device));
  HIPCHK(hipStreamSynchronize(src->stream));   // the shared arrays are complete
  bwgr_panel *P = new bwgr_panel();
  P->data = src->data; P->data->nclones++;
  Guard drop([&] { bwgr_panel_destroy(P); });
  if (!(P->stream = P->own.stream(hipStreamNonBlocking, 0))) return fail(BWGR_EHIP, "panel_clone: no stream for the clone");
  CHK(scratch_alloc(P));
  HIPCHK(hipStreamSynchronize(P->stream));   // (k_sweep3's lists are zeroed on it)
  drop.release();
  *out = P;
  return BWGR_OK;
}

extern "C" int bwgr_panel_set_stream(bwgr_panel *P, void *hip_stream) {
  if (!P) return fail(BWGR_EINVAL, "null panel");
  P->stream = reinterpret_cast<hipStream_t>(hip_stream);
  P->pre_pair_set = false;   // (the caller's choice stands: no return to an earlier stream)
  return BWGR_OK;
}

extern "C" int bwgr_panel_info(const bwgr_panel *P, int64_t info[8]) {
  if (!P || !info) return fail(BWGR_EINVAL, "null pointer");
  info[0] = P->data->n; info[1] = P->data->p; info[2] = P->data->plan.ld; info[3] = P->data->plan.m; info[4] = P->data->plan.K; info[5] = P->data->plan.R;
  info[6] = (int64_t)P->data->plan.x_bytes; info[7] = (int64_t)(2 * P->data->plan.gram_bytes);
  return BWGR_OK;
}

extern "C" int bwgr_panel_stats(bwgr_panel *P, float *xx, float *vx, float *MSx) {
  if (!P) return fail(BWGR_EINVAL, "null panel");
  HIPCHK(hipSetDevice(P->data->device));
  if (xx) HIPCHK(d2h(P->stream, xx, P->data->cen ? P->data->xxc : P->data->xx, sizeof(float) * P->data->p));   // (centred panel: the centred columns' norms)
  if (vx) HIPCHK(d2h(P->stream, vx, P->data->vx, sizeof(float) * P->data->p));
  if (MSx) *MSx = P->data->MSx;
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// what the families' entries share beside the sweep: the row gather, the redo count of the entries without a chain, X * coef, centring
// ------------------------------------------------------------------------------------------------
// The row gather's path, decided here and nowhere else (bwgr_debug_aux_plan exposes it to the CPU tests): 0 = element-wise (float panels, int8
// columns longer than 64 KB), else the columns an int8 workgroup stages in LDS -- ~30 KB of LDS per workgroup: five of them per CU
static int gather_mpw(bool is_f32, int64_t ld) {
  if (is_f32 || ld > 64 * 1024) return 0;
  return (int)std::max<int64_t>(1, std::min<int64_t>(8, (32 * 1024) / ld));
}
static size_t gather_lds(int mpw, int64_t ld) { return (size_t)mpw * (size_t)ld; }   // the staged columns
// row gather of the resident panel P into the subsample panel PB (rows use_d[0..nbag), device array); KMUP2's H = X(Use, j)
static void launch_gather_rows(bwgr_panel *P, bwgr_panel *PB, const int *use_d, int64_t nbag) {
  const int mpw = gather_mpw(P->data->is_f32, P->data->plan.ld);
  if (P->data->is_f32) hipLaunchKernelGGL(k_gather_rows<float>, dim3(4096), dim3(256), 0, P->stream, (const float *)P->data->X, P->data->plan.R, use_d, (int)nbag, (float *)PB->data->X, PB->data->plan.R, PB->data->plan.ld, P->data->p);
  else if (mpw > 0) {   // a column fits the LDS: stage, pick, write in 16-byte pieces
    hipLaunchKernelGGL(k_gather_rows_i8, dim3((unsigned)((P->data->p + mpw - 1) / mpw)), dim3(256), gather_lds(mpw, P->data->plan.ld), P->stream, (const int8_t *)P->data->X, P->data->plan.R, P->data->plan.ld,
                       use_d, (int)nbag, (int8_t *)PB->data->X, PB->data->plan.R, PB->data->plan.ld, P->data->p, mpw);
  } else hipLaunchKernelGGL(k_gather_rows<int8_t>, dim3(4096), dim3(256), 0, P->stream, (const int8_t *)P->data->X, P->data->plan.R, use_d, (int)nbag, (int8_t *)PB->data->X, PB->data->plan.R, PB->data->plan.ld, P->data->p);
}

// Sweeps that the calling thread's last bwgr_kmup / bwgr_kmup2 / bwgr_wgr / bwgr_wgr_ex call redid on the fp64 residual after they left the
// fixed-point range (test hook: those entry points have no chain to ask, bwgr_chain_redo_count)
static thread_local int g_last_redo = 0;
extern "C" int bwgr_debug_last_redo(int *count) {
  if (!count) return fail(BWGR_EINVAL, "null pointer");
  *count = g_last_redo;
  return BWGR_OK;
}

// column chunks of the two-stage GEMV: enough workgroups to fill the chip at 16 rows per thread (int8) or 4 (float)
// (the rule, the columns of a chunk and the row workgroups live in the three functions below and nowhere else: bwgr_debug_aux_plan exposes them)
static int gemv_chunks_of(bool is_f32, int64_t p) { return (int)std::min<int64_t>(is_f32 ? 64 : 512, std::max<int64_t>(1, p / 512)); }
static int gemv_cpc_of(int64_t p, int nchunks) { return (int)((p + nchunks - 1) / nchunks); }
static unsigned gemv_row_wgs(bool is_f32, int64_t ld) { return (unsigned)((ld / (is_f32 ? 4 : 16) + 255) / 256); }
static int gemv_chunks(const bwgr_panel *P) { return gemv_chunks_of(P->data->is_f32, P->data->p); }
// The two launch rules without a device (test hook).  out: see include/bwgr.h.
extern "C" int bwgr_debug_aux_plan(int is_f32, int64_t p, int64_t ld, int64_t out[BWGR_AUX_PLAN_NOUT]) {
  if (!out || p < 1 || ld < 128 || ld % 128) return fail(BWGR_EINVAL, "debug_aux_plan: null pointer, p < 1 or ld not a positive multiple of 128");
  const int nchunks = gemv_chunks_of(is_f32 != 0, p), mpw = gather_mpw(is_f32 != 0, ld);
  const int64_t v[BWGR_AUX_PLAN_NOUT] = {nchunks, gemv_cpc_of(p, nchunks), (int64_t)gemv_row_wgs(is_f32 != 0, ld), mpw, (int64_t)gather_lds(mpw, ld)};
  std::copy(v, v + BWGR_AUX_PLAN_NOUT, out);
  return BWGR_OK;
}
template <typename CT>
static void gemv_launch(bwgr_panel *P, const CT *coef_dev, int nchunks, int cpc, double *part) {
  if (P->data->is_f32) {
    dim3 grid(gemv_row_wgs(true, P->data->plan.ld), (unsigned)nchunks);
    hipLaunchKernelGGL((k_gemv_part<float, CT>), grid, dim3(256), 0, P->stream, (const float *)P->data->X, P->data->plan.ld, P->data->plan.R, (int)P->data->p, coef_dev, cpc, part);
  } else {
    dim3 grid(gemv_row_wgs(false, P->data->plan.ld), (unsigned)nchunks);
    hipLaunchKernelGGL((k_gemv_part_i8<CT>), grid, dim3(256), 0, P->stream, (const int8_t *)P->data->X, P->data->plan.ld, P->data->plan.R, (int)P->data->p, coef_dev, cpc, part);
  }
}

// hat = X*B + MU   (src/Rcpp20260726ai.cpp:629-630), fp64 accumulation, deterministic two-stage
template <typename CT>
static int gemv_hat(bwgr_panel *P, const CT *coef_dev, float MU, float *hat_dev, const char *who, bool centred = false) {
  const int nchunks = gemv_chunks(P);
  const int cpc = gemv_cpc_of(P->data->p, nchunks);
  DevBufs bufs;
  double *part = bufs.get<double>((size_t)nchunks * P->data->plan.ld + 1);
  if (!part) return fail(BWGR_ENOMEM, "%s: device allocation failed", who);
  gemv_launch<CT>(P, coef_dev, nchunks, cpc, part);
  double *cen_off = nullptr;
  if constexpr (std::is_same<CT, float>::value) {
    if (centred) {   // X_c B = X B - sum_j mean_j B_j
      cen_off = part + (size_t)nchunks * P->data->plan.ld;
      hipLaunchKernelGGL(k_cen_dot, dim3(1), dim3(1024), 0, P->stream, P->data->csum, coef_dev, P->data->p, 1.0 / (double)P->data->n, cen_off);
    }
  }
  hipLaunchKernelGGL(k_hat_finish, dim3((unsigned)((P->data->n + 255) / 256)), dim3(256), 0, P->stream, part, P->data->plan.ld, nchunks, (int)P->data->n, MU, hat_dev, (const double *)cen_off);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(P->stream));
  return BWGR_OK;
}

// Sweep the IMPLICITLY centred columns x_j - mean(x_j) of an int8 panel from now on (on != 0) or the raw columns again (on == 0): nothing is
// converted or copied -- the genotypes stay int8, the streamers, Gram arrays and MFMA tiles stay those of the raw columns, and the sequencer of
// k_sweep3 carries the scalar terms (sweep3.hip.h, "implicitly centred sweeps").  What changes for the callers: bwgr_panel_stats returns the centred
// columns' squared norms, the fused chains (bwgr_chain_*, bwgr_bayes, bwgr_group_*) run the reference's sweep on the centred columns
// (src/Rcpp20260726ai.cpp:668-682 with X_j - mean_j for X_j; selection models on k_sweep3 only), hat = X_c B + mu, and bwgr_panel_centred answers 1 -- which is
// what makes the marker-sharded sampler of several devices sound without a float copy of the panel.  Refused while chains are alive.
extern "C" int bwgr_panel_set_centred(bwgr_panel *P, int on) {
  if (!P) return fail(BWGR_EINVAL, "null panel");
  if (!P->is_root) return fail(BWGR_EINVAL, "panel_set_centred: set it on the root panel (clones follow it)");
  if (P->data->nchains_all > 0) return fail(BWGR_EINVAL, "panel_set_centred: %d chains are alive on this panel and its clones", P->data->nchains_all);
  HIPCHK(hipSetDevice(P->data->device));
  if (!on) { P->data->cen = false; return BWGR_OK; }
  if (P->data->is_f32) return fail(BWGR_EINVAL, "panel_set_centred: float panels are swept as given (centre the columns before the upload)");
  if (!P->data->e3_ready) return fail(BWGR_EINVAL, "panel_set_centred: this panel has no k_sweep3 (geometry or Gram range): the implicitly centred sweep is k_sweep3's");
  if (!P->data->csum) {   // the panel gets the pair once both arrays exist and are filled
    int32_t *csum = nullptr; float *xxc = nullptr;
    if (!P->data->own.take({{&csum, sizeof(int32_t) * (size_t)P->data->p}, {&xxc, sizeof(float) * (size_t)P->data->p}})) return no_memory("panel_set_centred");
    Guard drop([&] { P->data->own.drop(csum); P->data->own.drop(xxc); });
    const int wpb = 4;
    hipLaunchKernelGGL(k_colsum_i8, dim3((unsigned)((P->data->p + wpb - 1) / wpb)), dim3(64 * wpb), 0, P->stream, (const int8_t *)P->data->X, P->data->plan.R, (int)P->data->n, (int)P->data->p, csum, xxc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(P->stream));
    drop.release();
    P->data->csum = csum; P->data->xxc = xxc;
  }
  P->data->cen = true;
  return BWGR_OK;
}

// ---- are a panel's columns centred?  The marker-sharded partitioned sampler is statistically sound only then (DESIGN.md section 8:
// uncentred genotypes are all collinear through the mean direction, every shard corrects the same stale residual mean and the summed
// corrections overshoot; on centred columns 2 / 4 / 8 shards follow the exact chain: tools/centred_shard_probe.py).  From the panel's
// own statistics: mean_j^2 = (xx_j - (n - 1) vx_j) / n; a column counts as centred when |mean_j| <= 1e-3 sd_j. ----
extern "C" int bwgr_panel_centred(bwgr_panel *P, int *centred) {
  if (!P || !centred) return fail(BWGR_EINVAL, "null pointer");
  if (P->data->cen) { *centred = 1; return BWGR_OK; }   // implicitly centred: exactly
  HIPCHK(hipSetDevice(P->data->device));
  DevBufs bufs;
  int *flag = bufs.get<int>(1), h = 0;
  if (!flag) return fail(BWGR_ENOMEM, "panel_centred: device allocation failed");
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), P->stream));
  hipLaunchKernelGGL(k_uncentred, dim3(256), dim3(256), 0, P->stream, P->data->xx, P->data->vx, P->data->p, (double)P->data->n, flag);
  HIPCHK(d2h(P->stream, &h, flag, sizeof(int)));
  *centred = h ? 0 : 1;
  return BWGR_OK;
}
