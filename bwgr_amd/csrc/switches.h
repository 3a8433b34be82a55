// bwgr_amd/csrc/switches.h -- the environment switches of libbwgr_hip.so: Switches and read_switches.  Plain C++17, no HIP: the panel and sweep
// plans take a Switches by reference, so a host-only caller (the plan hooks) reads the environment exactly as bwgr_panel_create does.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

// The environment switches, every one the library reads, read once: when a root panel is made.  Clones share the
// root's; the scratch panels of KMUP2, bagging and the EM family, and groups take the panels' they are made for.  First-character switches
// hold that character (-1: unset); numeric ones hold their value as parsed (0: unset); the rest their parsed meaning.
struct Switches {
  int sweep = -1, lag = -1, solo3 = -1, stream3 = -1, pf3 = -1;                  // BWGR_SWEEP, BWGR_LAG, BWGR_SOLO3, BWGR_STREAM3, BWGR_PF3
  int r3 = 0, d3 = 0, nfeed = 0, sh_add = 0, max_concurrent = 0, max_pairs = 0;  // BWGR_R3, BWGR_D3, BWGR_NFEED, BWGR_DEBUG_SH_ADD, BWGR_MAX_CONCURRENT, BWGR_MAX_PAIRS
  // BWGR_ENG3_THR: k_sweep3 takes the sweeps whose chains hold fewer than this share of markers in the model; measured crossover at n = 10 000:
  // us per block at 1.4 / 3.7 / 5.8 / 10.9 % inclusion: k_sweep3 2.26 / 3.73 / 5.56 / 12.1, k_sweep2 3.07 / 3.29 / 3.60 / 4.69
  float eng3_thr = 0.03f;
  bool occ_guard = true, pf3b = true, draws = true, gram16 = true;   // BWGR_OCC_GUARD=0, BWGR_PF3B=0, BWGR_DRAWS=0, BWGR_GRAM16=0 switch these off
  // BWGR_WINV=0: the serial recurrence of k_sweep2's sequencer instead of k_sweep2w; BWGR_WFX=0: k_sweep2's streamers under its product sequencer
  // instead of the fixed-point ones; BWGR_WPF / BWGR_WAHEAD / BWGR_WNQ (0: by the streamer count) / BWGR_WLAG (=5|6: distances 4 / 5 through LDS
  // planes -- measured slower: C4-shape BayesA 22.3 / 23.0 / 24.9 ms per sweep at depth 4 / 5 / 6)
  bool winv = true, wfx = true;
  // BWGR_FIXED3=0: k_sweep3 also where a launch matches k_sweep3f, the fixed-shape instantiation (plan_sweep).  The experiment build (-DBWGR_EXPERIMENTS)
  // takes k_sweep3f only when asked, BWGR_FIXED3=1: tools/ab3_probe.py times either one under the BWGR_DBG3 switches.
#ifdef BWGR_EXPERIMENTS
  bool fixed3 = false;
#else
  bool fixed3 = true;
#endif
  int wpf = 4, wahead = 5, wnq = 0, wlag_cap = 4;
  bool group_allow_uncentred = false, group_force_comm = false, em_debug = false;   // BWGR_GROUP_ALLOW_UNCENTRED=1, BWGR_GROUP_FORCE_COMM=1, BWGR_EM_DEBUG
  int64_t kchunk = 0;   // BWGR_KCHUNK: markers per int32 chunk of the X X' product (0: the largest that keeps the int32 sums exact, plan_xxt)
#ifdef BWGR_EXPERIMENTS
  int dbg3 = 0, dbgw = 0, wlag_timing = 0; bool no_recover = false;   // BWGR_DBG3, BWGR_DBGW, BWGR_WLAG_TIMING, BWGR_NO_RECOVER
#endif
};
static Switches read_switches() {
  const auto chr = [](const char *v) { return v ? (int)(unsigned char)v[0] : -1; };
  const auto num = [](const char *v) { return v ? atoi(v) : 0; };
  Switches s;
  s.sweep = chr(getenv("BWGR_SWEEP")); s.lag = chr(getenv("BWGR_LAG")); s.solo3 = chr(getenv("BWGR_SOLO3"));
  s.stream3 = chr(getenv("BWGR_STREAM3")); s.pf3 = chr(getenv("BWGR_PF3"));
  s.r3 = num(getenv("BWGR_R3")); s.d3 = num(getenv("BWGR_D3")); s.nfeed = num(getenv("BWGR_NFEED")); s.sh_add = num(getenv("BWGR_DEBUG_SH_ADD"));
  s.max_concurrent = num(getenv("BWGR_MAX_CONCURRENT")); s.max_pairs = num(getenv("BWGR_MAX_PAIRS"));
  if (const char *v = getenv("BWGR_ENG3_THR")) { const float t = (float)atof(v); if (t > 0.0f) s.eng3_thr = t; }
  s.occ_guard = chr(getenv("BWGR_OCC_GUARD")) != '0'; s.pf3b = chr(getenv("BWGR_PF3B")) != '0'; s.draws = chr(getenv("BWGR_DRAWS")) != '0';
  s.gram16 = chr(getenv("BWGR_GRAM16")) != '0';
  { const int c = chr(getenv("BWGR_FIXED3")); if (c == '0') s.fixed3 = false; else if (c == '1') s.fixed3 = true; }
  s.winv = chr(getenv("BWGR_WINV")) != '0'; s.wfx = chr(getenv("BWGR_WFX")) != '0';
  if (const char *v = getenv("BWGR_WPF")) s.wpf = std::max(0, std::min(8, atoi(v)));
  if (const char *v = getenv("BWGR_WAHEAD")) s.wahead = std::max(1, atoi(v));
  { const int v = num(getenv("BWGR_WNQ")), c = chr(getenv("BWGR_WLAG")); if (v == 1 || v == 2 || v == 4) s.wnq = v; if (c >= '2' && c <= '6') s.wlag_cap = c - '0'; }
  s.group_allow_uncentred = chr(getenv("BWGR_GROUP_ALLOW_UNCENTRED")) == '1'; s.group_force_comm = chr(getenv("BWGR_GROUP_FORCE_COMM")) == '1';
  s.em_debug = getenv("BWGR_EM_DEBUG") != nullptr;
  if (const char *v = getenv("BWGR_KCHUNK")) s.kchunk = std::max<long long>(0, atoll(v));
#ifdef BWGR_EXPERIMENTS
  s.dbg3 = num(getenv("BWGR_DBG3")); s.dbgw = num(getenv("BWGR_DBGW")); s.wlag_timing = num(getenv("BWGR_WLAG_TIMING"));
  s.no_recover = getenv("BWGR_NO_RECOVER") != nullptr;
#endif
  return s;
}
