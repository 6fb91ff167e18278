// auv_multi_geom.h -- the launch geometry of k_step_multi (auv_step_multi): which workgroup order a slice takes, how lead / lag are
// clamped, how many workgroups the launch has, and which (step, role, index) each workgroup is.  One source for the kernel
// (k_step_fused.hip), its launcher and the C ABI's checks (auv_capi_step.hip); plain C++ without HIP headers, so that
// tests/test_multi_geometry.py compiles it with the host compiler and checks every decode of small launches and the division at
// every size the host accepts.
#pragma once

#if defined(__HIPCC__)
#define AUV_HD __host__ __device__
#else
#define AUV_HD
#endif

// workgroups of one cohort position: 8 dynamics + 64 sweep + 64 search + 8 finish
#define AUV_MULTI_COHORT_WG 144
// lanes per workgroup (AUV_WAVE)
#define AUV_MULTI_WG_LANES 64
// the dispatch packet's grid size is a 32-bit count of work-items (hipExtModuleLaunchKernel's globalWorkSizeX)
#define AUV_MULTI_MAX_ITEMS 0xffffffffull

// roles: 0 dynamics (8 environments per wave), 1 sweep, 2 search (one environment per wave), 3 finish (8 per wave)
struct AuvMultiWave {
  int step, role, bi;        // step == n_steps: the workgroup lies outside the launch and does nothing
};

struct AuvMultiGeom {
  int ne, n_steps;
  int lead, lag;             // cohort order: clamped lead / lag; step-major order: lead = -1, lag = 0
  unsigned magic;            // cohort order: ceil(2^32 / C); step-major order: 0
};

AUV_HD inline int auv_multi_dyn_waves(int ne) { return 8 * ((ne + 63) / 64); }       // nk: dynamics (= finish) waves of a step
AUV_HD inline int auv_multi_env_waves(int ne) { return 8 * ((ne + 7) / 8); }         // nb: sweep (= search) workgroups of a step
AUV_HD inline int auv_multi_role_count(int ne, int role) { return (role == 0 || role == 3) ? auv_multi_dyn_waves(ne) : ne; }

// the cohort order needs whole cohorts of 64 environments, and at least 3 of them (lead, lag >= 1 and lead + lag <= C - 1)
AUV_HD inline bool auv_multi_cohorts_ok(int ne) { return ne % 64 == 0 && ne / 64 >= 3; }

// lead, lag >= 1 and lead + lag <= C - 1: the dynamics of q + C (position q + C) are dispatched after the finish waves of q
// (position q + lead + lag), so every producer is ahead of its consumer in dispatch order, also across steps
AUV_HD inline void auv_multi_clamp(int C, int* lead, int* lag) {
  if (*lead < 1) *lead = 1;
  if (*lag < 1) *lag = 1;
  while (*lead + *lag > C - 1) {
    if (*lag > *lead && *lag > 1) (*lag)--;
    else if (*lead > 1) (*lead)--;
    else (*lag)--;
  }
}

AUV_HD inline unsigned auv_multi_magic(int C) { return (unsigned)((0x100000000ull + (unsigned)C - 1u) / (unsigned)C); }

// q / C and q % C by the multiplier m = ceil(2^32 / C), for C >= 2 and q < 2^32.  m = (2^32 + e) / C with 0 <= e < C, so
// q * m / 2^32 = q / C + q * e / (C * 2^32) and the second term is below 1: the estimate is q / C or one more (when q * e is
// large enough: at C = 8191 first at q = 532414), and one correction makes it exact.
AUV_HD inline int auv_multi_div(unsigned q, int C, unsigned magic, int* rem) {
  int s = (int)(((unsigned long long)q * magic) >> 32);
  int r = (int)q - s * C;
  if (r < 0) s--, r += C;
  *rem = r;
  return s;
}

AUV_HD inline AuvMultiGeom auv_multi_geom(int ne, int n_steps, int order, int lead, int lag) {
  AuvMultiGeom g;
  g.ne = ne, g.n_steps = n_steps;
  if (order == 1 && auv_multi_cohorts_ok(ne)) {
    const int C = ne / 64;
    auv_multi_clamp(C, &lead, &lag);
    g.lead = lead, g.lag = lag, g.magic = auv_multi_magic(C);
  } else {
    g.lead = -1, g.lag = 0, g.magic = 0u;
  }
  return g;
}

// workgroups of the launch: step-major, the one-launch step's grid n_steps times over; cohort order, n_steps * C + lead + lag
// positions of 144
AUV_HD inline unsigned long long auv_multi_grid(const AuvMultiGeom& g) {
  if (g.lead < 0) return (unsigned long long)g.n_steps * (unsigned long long)(2 * auv_multi_dyn_waves(g.ne) + 2 * auv_multi_env_waves(g.ne));
  return ((unsigned long long)g.n_steps * (unsigned long long)(g.ne / 64) + (unsigned long long)(g.lead + g.lag)) * AUV_MULTI_COHORT_WG;
}

// what the host may launch: the grid in work-items within the dispatch packet's 32 bits (and so every position and q below 2^32)
AUV_HD inline bool auv_multi_fits(const AuvMultiGeom& g) { return auv_multi_grid(g) * AUV_MULTI_WG_LANES <= AUV_MULTI_MAX_ITEMS; }

// step-major: all of step t's workgroups, role by role (nk dynamics, nb sweeps, nb searches, nk finish), then step t + 1's
AUV_HD inline AuvMultiWave auv_multi_decode_steps(unsigned bx, int ne, int n_steps) {
  const int nk = auv_multi_dyn_waves(ne), nb = auv_multi_env_waves(ne);
  const unsigned per = (unsigned)(2 * nk + 2 * nb);
  AuvMultiWave w;
  w.step = (int)(bx / per);
  const int b = (int)(bx - (unsigned)w.step * per);
  w.role = b < nk ? 0 : (b < nk + nb ? 1 : (b < nk + 2 * nb ? 2 : 3));
  w.bi = b - (w.role == 0 ? 0 : (w.role == 1 ? nk : (w.role == 2 ? nk + nb : nk + 2 * nb)));
  if (w.step >= n_steps || w.bi >= auv_multi_role_count(ne, w.role)) w.step = n_steps;
  return w;
}

// cohort-pipelined (ne % 64 == 0, C = ne / 64 >= 3): a cohort = 64 consecutive environments = 8 dynamics + 64 sweep + 64 search
// + 8 finish workgroups.  Cohort-steps are numbered q = step * C + cohort; position p holds the dynamics of q = p, the sweeps
// and searches of q = p - lead and the finish waves of q = p - lead - lag.  (Called with any ne by the kernel, which computes
// both orders and selects one: the result is then unused, only the arithmetic must be harmless.)
AUV_HD inline AuvMultiWave auv_multi_decode_cohorts(unsigned bx, int ne, int n_steps, int lead, int lag, unsigned magic) {
  const int C = ne / 64;
  const int p = (int)(bx / AUV_MULTI_COHORT_WG), r = (int)(bx - AUV_MULTI_COHORT_WG * (unsigned)p);
  AuvMultiWave w;
  w.role = r < 8 ? 0 : (r < 72 ? 1 : (r < 136 ? 2 : 3));
  const int q = p - (w.role == 0 ? 0 : (w.role == 3 ? lead + lag : lead));
  const bool q_ok = q >= 0 && q < n_steps * C;
  int c = 0;
  w.step = q_ok ? auv_multi_div((unsigned)q, C, magic, &c) : n_steps;
  w.bi = (w.role == 0 ? r : (w.role == 1 ? r - 8 : (w.role == 2 ? r - 72 : r - 136))) + ((w.role == 0 || w.role == 3) ? 8 * c : 64 * c);
  return w;
}
