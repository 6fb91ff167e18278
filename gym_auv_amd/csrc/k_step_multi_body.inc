// k_step_multi_body.inc -- the body of a launch of several steps, included by csrc/k_step_fused.hip once per kernel:
//   STEP_MULTI_REC 0   k_step_multi   every step writes the same obs / reward / done rows (the last step's remain)
//   STEP_MULTI_REC 1   k_step_record  step k of the launch writes its rows `k * stride` elements further on: a [T][N] record
//   STEP_MULTI_FB 1    k_step_feedback (recording on)  the action of step t is the affine feedback law of the OBS64 row step t - 1
//                      left (fb_law, k_step_fused.hip): step 0's dynamics wave forms it from the arrays, every later step's takes it
//                      from words 21..23 of the carry record, where the previous step's finish wave has put it.  Further
//                      parameters: gains ([N][2][8] fp64), act_rec ([T][N][2] fp64 or nullptr); `actions` may be nullptr (x_7 = 0).
//   STEP_MULTI_FB 2    k_step_sector_feedback  the same with LiDAR sector inputs in the law (fb_sector_pair, fb_law_sectors): further
//                      parameters sgains ([N][2][16] fp64) and sb (FbBounds by value, the sector bounds).
//   STEP_MULTI_FB 3    k_step_hidden_feedback  the same with one hidden layer of 16 units over the law's 24 inputs (fb_hidden): further
//                      parameters hidden ([N][16][28] fp64) and activation (0 relu, 1 hard tanh).
//   STEP_MULTI_FW 1    k_fresh_multi / k_fresh_record (REC 0 / 1, FB 0)  a fresh world per reset: the finish wave's reset binds the
//                      environment's next slot only if it was published before this call began (auv_next_world_multi).  Further
//                      parameter: fw_call, the call's number.  (Not defined by the other inclusions: `#if` reads it as 0.)
//   STEP_MULTI_FB 1 / 2 / 3 with STEP_MULTI_FW 1   k_fresh_feedback / k_fresh_sector_feedback / k_fresh_hidden_feedback (REC 1): the
//                      closed-loop launch on a fresh world per reset; the closed-loop kernel's parameters, then fw_call.  The finish
//                      role's branches for them stand in front of the others, whose text is as it was.
// The includer has declared `d` (AUV_KERNARG_DESC) and the kernel's parameters: actions, obs_out, reward_out, done_out, n_steps,
// first_slot, n_slots, seq0, lead_dyn, lag_fin, magic_c -- and, recording, obs_stride, reward_stride, done_stride (elements; 0: no
// record of that output).  The record's offset is wave-uniform (the step is, the strides are kernel arguments): 64-bit scalar
// arithmetic once per wave, and every writer -- the sweep's closeness columns, the tail's navigation features, the reward phase, a
// restored environment's row -- keeps its code and its GLOBAL environment index.
// (Text, not a function template on `bool REC` inlined into two wrappers: that was tried first and k_step_multi's code came out
// different -- same register counts, other allocation and block layout -- where this change is meant to leave it alone.)
  extern __shared__ __align__(16) unsigned char smem[];
#ifdef AUV_STAMPS_MULTI
  const unsigned long long t_entry = wall_clock64();      // the wave's first instruction
#endif
  const int lane = threadIdx.x;
  const int ne = d.ne;
  // role: 0 dynamics, 1 sweep, 2 search, 3 finish; bi: the wave's index within its role and step (auv_multi_geom.h: the decode,
  // the launcher's grid and the host's checks have this one source).
  // Two workgroup orders (both computed, one selected: a run-time branch around this index arithmetic makes this compiler emit a
  // vector-to-scalar copy it then rejects):
  //   step-major: all of step t's workgroups, role by role, then step t + 1's;
  //   COHORT-PIPELINED (lead_dyn >= 0).  A cohort = 64 consecutive environments = 8 dynamics + 64 sweep + 64 search + 8 finish
  //   workgroups (every run a multiple of 8: an environment's waves still share an XCD).  Cohort-steps are numbered
  //   q = step * C + cohort; position p of the grid holds the dynamics of q = p, the sweeps and searches of q = p - lead and the
  //   finish waves of q = p - lead - lag: a sweep is dispatched `lead` positions behind its dynamics -- which have finished by
  //   then -- and a finish wave `lag` positions behind its sweeps, so waves find what they need instead of holding a slot while
  //   they poll for it (the step-major order makes step t + 1's sweeps wait, resident, for a finish wave that is dispatched last
  //   of all of step t).  lead + lag < C keeps every producer ahead of its consumer in index order, also across steps: the
  //   dynamics of q + C sit at position q + C, behind the finish waves of q at q + lead + lag.
  // A workgroup outside the launch -- past the last step, or past its role's count (a slice that is not a multiple of 8
  // environments) -- decodes to step == n_steps and ends here.
  const bool cohorts = lead_dyn >= 0;
  const AuvMultiWave wa = auv_multi_decode_steps(blockIdx.x, ne, n_steps);
  const AuvMultiWave wc = auv_multi_decode_cohorts(blockIdx.x, ne, n_steps, lead_dyn, lag_fin, magic_c);
  const int step = auv_uniform(cohorts ? wc.step : wa.step);
  const int role = auv_uniform(cohorts ? wc.role : wa.role), bi = auv_uniform(cohorts ? wc.bi : wa.bi);
  if (step >= n_steps) return;
#if STEP_MULTI_REC
  {
    // this step's rows of the record (a stride of 0: no record of that output, every step writes the one row)
    obs_out += (unsigned long long)(unsigned)step * obs_stride;
    reward_out += (unsigned long long)(unsigned)step * reward_stride;
    done_out += (unsigned long long)(unsigned)step * done_stride;
  }
#endif
  const unsigned long long tagmix = roles_tagmix(seq0 + (unsigned long long)step + 1ull), tagmix_prev = roles_tagmix(seq0 + (unsigned long long)step);
#ifdef AUV_STAMPS_MULTI
  unsigned long long* const stamp = d.stamps + (step == n_steps / 2 ? (size_t)0 : (size_t)16 * (size_t)d.n);
#endif
  if (role == 0) {
    // ---- Vessel.step of eight environments ----
    __builtin_amdgcn_s_setprio(3);
    const int b = bi;
    const int g = lane / K1_GROUP, c = lane % K1_GROUP;
    const int er = 8 * (8 * (b / 8) + g) + (b % 8);
    const bool live = er < ne;
    const int eg = d.e0 + (live ? er : ne - 1);
    int y, gave_up = 0;
    double y0 = 0.0;
    MSTAMP_IF(live && c == 0, eg, 10);
    // requested ahead of the wait for the carry record (this wave is on every environment's critical path): the flag and the action
    const int ab_early = __hip_atomic_load(d.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    double act0, act1;
#if STEP_MULTI_FB
    // (only step 0 forms the law here and needs the ring's action, x_7, for it: later steps' came with the carry record)
    act0 = act1 = 0.0;
    if (step == 0 && actions) k1_action(d, actions, eg, &act0, &act1, first_slot % n_slots);
    unsigned long long v2 = 0ull;
#else
    k1_action(d, actions, eg, &act0, &act1, (first_slot + step) % n_slots);
#endif
    if (step == 0) {
      y = d.counters[eg].y + 1;
#if STEP_MULTI_FB
      // the arrays, behind the kernel boundary: the OBS64 row and the gains
      const double x = c < 6 ? d.obs64[(size_t)eg * (6 + d.cfg.n_sensors) + c] : 0.0;
#if STEP_MULTI_FB == 3
      double2 a = fb_law(c, x, gains[16 * (size_t)eg + c], gains[16 * (size_t)eg + 8 + c], act0, act1);
      {
        const double* hp = sgains + 32 * (size_t)eg + c;
        const double2 h0 = make_double2(hp[0], hp[8]), h1 = make_double2(hp[16], hp[24]);
        const double* wp = hidden + (size_t)(16 * FB_HIDDEN_ROW) * (size_t)eg + FB_HIDDEN_ROW * c;
        const FbHiddenBatch w0 = fb_hidden_request<0>(wp);
        const FbHiddenTail wt = fb_hidden_request_tail(wp);
        const double2 z = fb_sector_pair<false>(d.obs64 + (size_t)eg * (6 + d.cfg.n_sensors) + 6, fb_ranges(sb, c));
        a = fb_hidden(fb_law_sectors(a, z, h0, h1), x, act0, act1, z, w0, wt, wp, activation);
      }
#elif STEP_MULTI_FB == 2
      double2 a = fb_law(c, x, gains[16 * (size_t)eg + c], gains[16 * (size_t)eg + 8 + c], act0, act1);
      {
        const double* hp = sgains + 32 * (size_t)eg + c;
        const double2 h0 = make_double2(hp[0], hp[8]), h1 = make_double2(hp[16], hp[24]);
        const double2 z = fb_sector_pair<false>(d.obs64 + (size_t)eg * (6 + d.cfg.n_sensors) + 6, fb_ranges(sb, c));
        a = fb_law_sectors(a, z, h0, h1);
      }
#else
      const double2 a = fb_law(c, x, gains[16 * (size_t)eg + c], gains[16 * (size_t)eg + 8 + c], act0, act1);
#endif
      act0 = a.x, act1 = a.y;
#endif
    } else {
      // this environment's state and counters after the previous step: the first line of its carry record
      const unsigned long long* cw = d.carry + CARRY_WORDS * (size_t)eg;
      unsigned long long v = 0ull;
      bool ok = !live;
      for (int polls = 0;; polls++) {
#if STEP_MULTI_FB
        // words 16 + c with words c, one more load in the same trip: lanes 5, 6, 7 then hold the action and its mark, and the
        // record is taken only when BOTH marks belong to the previous step
        if (!ok) v = __hip_atomic_load(cw + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), v2 = __hip_atomic_load(cw + 16 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = !live || (roles_record_ok(v, c, tagmix_prev) && fb_record_ok(v2, c, tagmix_prev));
#else
        if (!ok) v = __hip_atomic_load(cw + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = !live || roles_record_ok(v, c, tagmix_prev);
#endif
        if (!__any(!ok)) break;
        if ((polls & 31) == 31 && auv_uniform(__hip_atomic_load(d.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
          gave_up = 1;                                                              // (ABORT packets below)
          break;
        }
        if (polls == (AUV_HOOK_FAULT(d) ? (1 << 12) : PAIR_POLL_LIMIT)) {
          if (live && c == 0) auv_st<true>(d.broken + eg, (uint8_t)1);
          roles_give_up(d, d.e0, d.ne, 6, lane);
          gave_up = 1;                                                              // (the flag is up now: ABORT packets below)
          break;
        }
        __builtin_amdgcn_s_sleep(ROLES_POLL_SLEEP);
      }
      y0 = __longlong_as_double((long long)v);
      y = (int)(unsigned)(roles_group_word(v, 6) >> 32) + 1;
#if STEP_MULTI_FB
      act0 = roles_group_value(v2, 5), act1 = roles_group_value(v2, 6);
#endif
    }
    const int aborted = gave_up | auv_uniform(ab_early);
    double t = 0.0;
    MSTAMP_IF(live && c == 0, eg, 11);
    const double2 act = make_double2(act0, act1);
    if (!aborted) t = k1_group(d, actions, eg, lane, step != 0, y0, (first_slot + step) % n_slots, &act);
#if STEP_MULTI_FB
    // the action record: `a` as the law gives it (the NaN rule and the clip are the dynamics'); a plain store, never waited for
    if (act_rec && live && !aborted && c < 2) act_rec[2 * ((size_t)step * (size_t)d.n + (size_t)eg) + c] = c == 0 ? act0 : act1;
#endif
    unsigned long long* pk = d.k1_pkt + 8 * (size_t)eg;
    const unsigned long long word = aborted ? (c == 6 ? (unsigned long long)ROLES_ABORT_COUNTER : 0ull)
                                            : (c < 6 ? (unsigned long long)__double_as_longlong(t) : (c == 6 ? (unsigned long long)(unsigned)y : 0ull));
    const unsigned long long mark = roles_mark(roles_group_xor(word) ^ tagmix);
    if (live && !(AUV_HOOK_FAULT(d) == 2 && eg == d.e0 && step == 0))
      __hip_atomic_store(pk + c, c < 7 ? word : mark, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    MSTAMP_IF(live && c == 0, eg, 12);
    return;
  }
  EnvPre pre;
  EnvDesc ed;
  if (role == 1) {
    // ---- _update + Vessel.perceive of one environment ----
    const int e = auv_uniform(d.e0 + bi);
    MSTAMP(e, 0);
    // four requests in flight before the first wait: the abort flag, this step's state packet (dispatched `lead` cohorts behind
    // its dynamics, the wave usually finds it there), the first look at the carry record (step 0 reads the arrays and drops it), and
    // behind those -- its addresses take two scalar loads more -- the beam table on its way straight into the ray slots (no
    // register waits for it: k2_stage_beams_direct).
    // (The wait in front of them finds nothing outstanding: a wave has requested nothing from memory before its role begins.  It
    // is there for the compiler, which otherwise assumes loads of the other roles still in flight here and waits for them, that is
    // for the abort flag's whole trip, in the middle of these requests.)
    __builtin_amdgcn_s_waitcnt(AUV_WAITCNT_VMCNT0);       // (a later toolchain may not need it: the sweep's head in the assembly tells)
    const int ab_early = __hip_atomic_load(d.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long pk_first = __hip_atomic_load(d.k1_pkt + 8 * (size_t)e + (lane & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long cw_first = carry_request(d, e, lane);
    Slice L = carve_base(smem, d.cfg.n_sensors, d.k_max, d.m_max, d.seg_cap);   // (k2_back's lists: placed in front of k2_back)
    k2_stage_beams_direct(d, lane, L);
    K2Pre kp;
    if (step == 0) {
      ed = d.env_desc[e];
      pre.cnt = d.counters[e];
      pre.ed = &ed;
      if (auv_uniform(ab_early)) return;
      k2_movers<true>(d, e, lane, L, ed, 1);
      kp = k2_prefetch(d, e, lane, ed);
    } else {
      if (carry_wait_wave(d, e, lane, tagmix_prev, ed, pre.cnt, true, cw_first)) return;
      if (auv_uniform(ab_early)) return;
      pre.ed = &ed;
      k2_movers<true, true>(d, e, lane, L, ed, 1);
      kp = k2_prefetch<true>(d, e, lane, ed);
    }
    {
      const int ws = roles_wait_state(d, e, lane, pre, tagmix, true, pk_first);
      if (ws) {
        if (ws == 2 && ed.M > 0 && lane == 0) auv_st<true>(d.broken + e, (uint8_t)1);
        return;
      }
    }
    MSTAMP(e, 2);
    int2 lim0 = make_int2(INT32_MIN, INT32_MIN);
    const int n_act = k2_front<true>(d, e, lane, L, 1, &pre, 1, &kp, true, &lim0);
    k2_stage_and_pairs(d, L, lane, n_act, pre.s[2]);
    MSTAMP(e, 4);
    double term = 0.0;
    {
      const AuvDev* dp = &d;
      asm volatile("" : "+s"(dp));                         // (fetched here: nothing of this is held across the sweep)
      const __attribute__((address_space(4))) AuvDev* dc = (const __attribute__((address_space(4))) AuvDev*)dp;
      carve_hits(L, dc->cfg.n_sensors, dc->m_max, dc->seg_cap);
    }
    const int collision = k2_back<true>(d, e, lane, L, n_act, obs_out, &term, &lim0);
    pair_publish_lidar(d, e, lane, collision, term);
    MSTAMP(e, 5);
#ifdef AUV_STAMPS_MULTI
    if (lane == 0) stamp[(size_t)e * 16 + 1] = t_entry;
    __builtin_amdgcn_s_waitcnt(AUV_WAITCNT_VMCNT0);                    // every store of this wave has been acknowledged
    MSTAMP(e, 3);
#endif
  } else if (role == 2) {
    // ---- Vessel.navigate of one environment: the nearest-point search ----
    const int e = auv_uniform(d.e0 + bi);
    MSTAMP(e, 6);
    const unsigned long long pk_first = __hip_atomic_load(d.k1_pkt + 8 * (size_t)e + (lane & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (step == 0) {
      ed = d.env_desc[e];
      pre.cnt = d.counters[e];
    } else if (carry_wait_wave(d, e, lane, tagmix_prev, ed, pre.cnt)) {
      return;
    }
#ifdef AUV_STAMPS_MULTI
    if (lane == 0) stamp[(size_t)e * 16 + 7] = t_entry;
#endif
    pre.ed = &ed;
    if (roles_wait_state(d, e, lane, pre, tagmix, true, pk_first)) return;
    MSTAMP(e, 8);
    NavNear nr;
    int* list = (int*)smem;
    const NavSpec sp = nav_bounds(d, e, lane, list, pre.s[0], pre.s[1], &ed);
    nr = nav_nearest(d, e, lane, list, pre.s[0], pre.s[1], sp);
    roles_publish_search(d, e, lane, nr, tagmix);
    MSTAMP(e, 9);
  } else {
    // ---- navigation tail + reward / done / auto-reset of eight environments ----
    const int f = bi;
    __builtin_amdgcn_s_setprio(2);
#ifdef AUV_STAMPS_MULTI
    const int fer = 8 * (8 * (f / 8) + lane / K1_GROUP) + (f % 8);
    const bool fst = fer < ne && lane % K1_GROUP == 0;
#endif
    MSTAMP_IF(fst, d.e0 + fer, 13);
#if STEP_MULTI_FB == 3 && STEP_MULTI_FW
    roles_finish_wave_multi<true, 3, 1>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG, gains,
                                        actions, (first_slot + step + 1) % n_slots, sgains, &sb, hidden, activation, fw_call);
#elif STEP_MULTI_FB == 2 && STEP_MULTI_FW
    roles_finish_wave_multi<true, 2, 1>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG, gains,
                                        actions, (first_slot + step + 1) % n_slots, sgains, &sb, nullptr, 0, fw_call);
#elif STEP_MULTI_FB && STEP_MULTI_FW
    roles_finish_wave_multi<true, 1, 1>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG, gains,
                                        actions, (first_slot + step + 1) % n_slots, nullptr, nullptr, nullptr, 0, fw_call);
#elif STEP_MULTI_FB == 3
    roles_finish_wave_multi<true, 3>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG, gains,
                                     actions, (first_slot + step + 1) % n_slots, sgains, &sb, hidden, activation);
#elif STEP_MULTI_FB == 2
    roles_finish_wave_multi<true, 2>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG, gains,
                                     actions, (first_slot + step + 1) % n_slots, sgains, &sb);
#elif STEP_MULTI_FB
    roles_finish_wave_multi<true, true>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG, gains,
                                        actions, (first_slot + step + 1) % n_slots);
#elif STEP_MULTI_FW
    roles_finish_wave_multi<true, 0, 1>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG, nullptr,
                                        nullptr, 0, nullptr, nullptr, nullptr, 0, fw_call);
#else
    roles_finish_wave_multi<true>(d, f, lane, obs_out, reward_out, done_out, step, step == n_steps - 1, tagmix, tagmix_prev MSTAMP_ARG);
#endif
    MSTAMP_IF(fst, d.e0 + fer, 15);
  }
