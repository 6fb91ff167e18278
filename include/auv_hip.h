/* auv_hip.h — C ABI of the MI355X-native batched gym-auv step() path.
 *
 * The reference (krisbrud/gym-auv) is pure Python and has NO FFI layer of its own; the
 * boundary it offers for this path is the gym.Env surface
 *   reset()            gym_auv/environment.py:176-245
 *   step(action)       gym_auv/environment.py:292-366
 *   observe()          gym_auv/environment.py:247-290
 * so every entry point below cites the reference method whose per-environment work it
 * performs for a whole batch of N independent environments.  Plain pointers and sizes
 * only (no torch types); the Python side binds it with ctypes.
 *
 * Conventions
 *   - return 0 on success, negative AUV_E* on failure; text via auv_last_error().
 *   - "dev" pointers are device (HBM) pointers owned by the CALLER (e.g. torch tensors);
 *     the handle owns environment state, world bank and scratch.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  auv_step and the
 *     per-kernel entry points are stream-ordered: no allocation, no host sync, hipGraph
 *     capturable.
 *   - one handle per GPU, one host thread per handle (the reference env is single-threaded
 *     and non-re-entrant; nothing stronger is promised).
 *   - all arithmetic is IEEE fp64 ("f64"); obs/reward are additionally emitted as fp32
 *     because observation_space.dtype is float32 (environment.py:139-143).
 */
#ifndef AUV_HIP_H
#define AUV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AUV_ABI_VERSION 5

enum {
  AUV_OK = 0,
  AUV_EINVAL = -1,   /* bad argument / shape mismatch            */
  AUV_EHIP = -2,     /* a HIP runtime call failed                */
  AUV_ESTATE = -3,   /* call order violated (e.g. no worlds yet) */
  AUV_ENOMEM = -4
};

enum { AUV_REWARD_COLAV = 0, AUV_REWARD_PATHFOLLOW = 1 };       /* rewarder.py:143, :56 */
enum { AUV_CULL_REFERENCE = 0, AUV_CULL_EXACT = 1 };            /* sensor.py:74-97 vs :100-137 */
enum { AUV_OBS_RING = 0, AUV_OBS_FILLED = 1, AUV_OBS_MOVER = 2 };
enum { AUV_F32 = 0, AUV_F64 = 1 };

/* Mirrors the fields of gym_auv/config.py that step() reads. */
typedef struct auv_config {
  double dt;                      /* SimulationConfig.t_step_size        config.py:28  */
  double min_goal_distance;       /* EpisodeConfig.min_goal_distance     config.py:20  */
  double min_path_progress;       /* EpisodeConfig.min_path_progress     config.py:23  */
  double min_cumulative_reward;   /* EpisodeConfig.min_cumulative_reward config.py:16  */
  double sensor_range;            /* VesselConfig.sensor_range           config.py:65  */
  double vessel_width;            /* VesselConfig.vessel_width           config.py:41  */
  double look_ahead_distance;     /* VesselConfig.look_ahead_distance    config.py:45  */
  double thrust_max;              /* VesselConfig.thrust_max_auv         config.py:39  */
  double moment_max;              /* VesselConfig.moment_max_auv         config.py:40  */
  int32_t max_timesteps;          /* EpisodeConfig.max_timesteps         config.py:19  */
  int32_t n_sensors;              /* n_sectors * n_sensors_per_sector    config.py:75  */
  int32_t sensor_interval_load_obstacles;                             /* config.py:56  */
  int32_t use_lidar;              /* VesselConfig.use_lidar              config.py:52  */
  int32_t sensor_log_transform;   /* VesselConfig.sensor_log_transform   config.py:66  */
  int32_t rewarder;               /* AUV_REWARD_*                                      */
  int32_t test_mode;              /* BaseEnvironment(test_mode=)   environment.py:32   */
  int32_t cull_mode;              /* AUV_CULL_*                                        */
  int32_t auto_reset;             /* VecEnv semantics: a done env restarts on its next
                                     world of the bank inside the same step            */
  int32_t obs_channels;           /* 1: closeness only; 3: + two velocity channels, which the
                                     reference hard-wires to zero (sensor.py:159, config.py:80-91) */
} auv_config_t;

/* World bank: W pre-generated scenario instances in CSR form (host pointers; copied to HBM
 * by auv_load_worlds).  Built by gym_auv_amd.world from WorldSpec, i.e. from what the
 * reference's _generate() hands to Path/Vessel/obstacles (envs/movingobstacles.py:28-95).
 *
 *  path      dense polyline of Path._points (path.py:38-40) + cumulative arclength (the
 *            measure GEOS LineString.project walks), and the final PCHIP as per-interval
 *            power-basis coefficients (path.py:26-27).
 *  obstacles per obstacle {kind, seg_off, nseg, mover_idx} + static cull circle
 *            (obstacles.py:108-113, :125-127); static boundary segments (obstacles.py:
 *            101-106, :122-123) as (ax, ay, bx, by).
 *  movers    VesselObstacle parameters and reset-time state (obstacles.py:144-215).
 */
typedef struct auv_world_bank {
  int32_t n_worlds;
  /* path */
  const int64_t* poly_off;    /* [W+1]  vertex offsets                                  */
  const double* poly_xy;      /* [sum P][2]                                             */
  const double* poly_cum;     /* [sum P]   cum[j] = arclength at vertex j               */
  const int64_t* knot_off;    /* [W+1]  knot offsets (n_k knots -> n_k-1 intervals)     */
  const double* knot_s;       /* [sum n]                                                */
  const double* knot_coef;    /* [sum n][8] x:c0..c3 (highest power first), y:c0..c3;
                                  row i describes interval [s_i, s_{i+1}); last row of
                                  each world unused                                     */
  const double* world_scalar; /* [W][8] L, end_x, end_y, init_x, init_y, init_psi, 0, 0 */
  /* obstacles */
  const int64_t* obs_off;     /* [W+1]                                                  */
  const int32_t* obs_meta;    /* [sum K][4] kind, seg_off (into seg, absolute), nseg,
                                  mover index within the world (or -1)                  */
  const double* obs_cull;     /* [sum K][3] cx, cy, rho (static obstacles)              */
  int64_t n_seg;
  const double* seg;          /* [n_seg][4] ax, ay, bx, by                              */
  /* movers */
  const int64_t* mv_off;      /* [W+1]                                                  */
  const double* mv_param;     /* [sum M][4] width, pos0_x, pos0_y, n_vel                */
  const double* mv_init;      /* [sum M][4] pos_x, pos_y, heading, counter at reset     */
  const int64_t* mv_vtab_off; /* [sum M + 1] offsets into mv_vtab                       */
  const double* mv_vtab;      /* [.][2] per-tick velocities (length 1 = constant)       */
} auv_world_bank_t;

typedef struct auv_handle auv_handle_t;

/* Field ids for auv_read / auv_write (handle-owned device buffers, all fp64 unless noted):
 * copies between the handle and a caller buffer, stream-ordered.  Test/debug surface. */
enum {
  AUV_FIELD_STATE = 0,       /* [6][N]  x, y, psi, u, v, r   (Vessel._state, SoA)          */
  AUV_FIELD_LIDAR_D = 1,     /* [N][S]  Vessel._last_sensor_dist_measurements              */
  AUV_FIELD_OBS64 = 2,       /* [N][6+S] observation before the float32 cast.  Pooled (auv_set_obs_pooling): the
                                 stride stays 6+S; columns 6 .. 6+n_sectors-1 hold the sectors' closenesses and
                                 the rest stay 0                                                 */
  AUV_FIELD_REWARD64 = 3,    /* [N]                                                        */
  AUV_FIELD_INFO64 = 4,      /* [N][8] collision, reached_goal, goal_distance, progress,
                                 cumulative_reward, max_progress, vessel_arclength, sum of |cross-track
                                 error| [m] over the steps of the episode so far               */
  AUV_FIELD_WORLD_IDX = 5,   /* [N] int32                                                  */
  AUV_FIELD_COUNTERS = 6,    /* [N][4] int32: t_step, vessel step_counter, episodes, pad   */
  AUV_FIELD_MOVER_STATE = 7, /* [N][Mmax][4] pos_x, pos_y, heading, counter                */
  AUV_FIELD_NEARBY = 8,      /* [N][Kmax] uint8  cached Vessel._nearby_obstacles mask      */
  AUV_FIELD_EPISODE = 9,     /* [N][4] last finished episode: return, length, collision,
                                 reached_goal (fp64)                                        */
  AUV_FIELD_CULL_LIMITS = 10,/* [N][Kmax][2] int32 idx_min_ray, idx_max_ray (sensor.py:58-69)
                                 of the last sweep; INT32_MIN where not evaluated           */
  AUV_FIELD_NAV64 = 11,      /* [N][8] unclipped Vessel.navigate outputs: u, v, r,
                                 look_ahead_heading_error, heading_error, cross_track_error/100,
                                 path_direction, target_arclength        (vessel.py:518-536) */
  AUV_FIELD_COLLISION = 12,  /* [N] uint8  Vessel._collision                                */
  AUV_FIELD_STAMPS = 13,     /* [N][16] uint64 per-phase cycle counts; zeros unless the library
                                 was built with STAMPS=1 (diagnostic)                       */
  AUV_FIELD_BROKEN = 15,     /* [N] uint8  environments whose step a wave that gave up polling has left unfinished
                                 (all zero except between a hand-over time-out and the call that recovers)     */
  AUV_FIELD_FW_STATE = 16,   /* [W] int32  fresh-world mode only: 0 READY (unseen), 1 IN_USE, 2 STALE (queued / being rebuilt) */
  AUV_FIELD_FW_SERIAL = 17,  /* [W] int32  fresh-world mode only: the slot holds world number `serial` of its environment    */
  AUV_FIELD_SECTOR_D = 18,   /* [N][n_sectors] pooled observation only (0 bytes otherwise): the feasible distance of every
                                 sector behind the current observation row (vessel.py:556-557 "feasible_distances");
                                 after a reset / auto-reset those of the reset row. Read-only in spirit: writing it
                                 changes no observation                                                              */
  AUV_FIELD_STEP_INFO = 14   /* [N][4] the `info` dict of the last step() as the reference
                                 returns it (environment.py:336-340): collision, reached_goal,
                                 goal_distance, progress -- of the step that was taken, i.e. the
                                 terminal values for an env that has just been auto-reset      */
};

/* Create an environment batch of n_envs on device `device_id`.            (environment.py:29-164) */
int auv_create(const auv_config_t* cfg, int32_t n_envs, int32_t device_id, auv_handle_t** out);
int auv_destroy(auv_handle_t* h);

/* Upload a world bank (replaces any previous one).                 (BaseEnvironment._generate) */
int auv_load_worlds(auv_handle_t* h, const auv_world_bank_t* bank);

/* reset(): for every env whose mask byte is non-zero (mask_dev == NULL: all) bind it to
 * world_idx_dev[e] (NULL: keep current binding; initial binding is e % W), restore vessel /
 * mover state and counters, then compute the first observation.          (environment.py:176-245) */
int auv_reset(auv_handle_t* h, const uint8_t* mask_dev, const int32_t* world_idx_dev,
              float* obs_dev, void* stream);

/* step(): _update -> vessel.step -> observe -> reward -> done, for all N envs.
 * actions_dev: [N][2] (thrust, rudder) of action_dtype AUV_F32/AUV_F64, 8- / 16-byte aligned.
 * obs_dev [N][6+S] f32, reward_dev [N] f32, done_dev [N] u8.             (environment.py:292-366) */
int auv_step(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, float* obs_dev,
             float* reward_dev, uint8_t* done_dev, void* stream);

/* step() of the environments [e0, e0 + ne) only, enqueued on `stream`; the buffers are the same full-batch
 * [N][..] buffers auv_step takes (only the slice's rows are read / written).  Environments are independent
 * (environment.py:86-89), so sub-batches of one handle may be stepped on DIFFERENT streams concurrently: one
 * sub-batch's LiDAR sweeps then run under another's dynamics chain and navigation tail -- the batched analogue
 * of the reference's SubprocVecEnv workers stepping at their own pace (scripts/run.py:293-296; VecEnv
 * step_async / step_wait).  Results are bit-identical to auv_step over the same environments.  Ordering between
 * sub-batches and with the consumer of obs / reward / done is the CALLER's (stream order, events).  Eager only
 * (a captured graph steps the whole batch).                                                                  */
int auv_step_slice(auv_handle_t* h, int32_t e0, int32_t ne, const void* actions_dev, int32_t action_dtype,
                   float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);
/* The same for ALL sub-batches with one call: slice i = [bounds[i], bounds[i + 1]) goes to streams[i]
 * (bounds[0] = 0, bounds[n_slices] = N; HOST arrays).  One step of the whole batch as n_slices independent
 * launch chains -- what a VecEnv.step_async() of this handle enqueues.                                        */
int auv_step_pipelined(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                       const void* actions_dev, int32_t action_dtype, float* obs_dev, float* reward_dev,
                       uint8_t* done_dev);

/* SEVERAL steps of every slice in ONE launch per slice (open-loop stretches: the actions are resident).  actions_dev is a ring of
 * n_slots consecutive [N][2] buffers; step k of the call reads slot (first_slot + k) % n_slots.  The launch is the one-launch step's
 * grid n_steps times over, step-major: an environment's step k + 1 starts when ITS finish wave of step k is through -- no barrier
 * over the slice between two steps, no launch turn-around.  What the kernel boundary between two launches did is done by a
 * per-environment carry record (agent-scope stores / loads, checksummed, every mark carrying the step's number): csrc/
 * k_step_fused.hip, k_step_multi.  obs / reward / done hold the LAST step's values afterwards; everything else -- state, counters,
 * episode log, auto-reset -- is bit for bit what n_steps calls of auv_step_pipelined leave (tests/test_gpu_multi.py).  Needs the
 * one-launch shape for every slice and at most 64 obstacles per world; refused with a fresh world per reset.  Polls are bounded and
 * report like the one-launch step's (auv_health).  1 <= n_steps <= 1024, and every slice's launch within the dispatch limit of
 * 2^32 - 1 work-items (64 per workgroup): step-major, n_steps * (2 * 8 * ceil(ne / 64) + 2 * 8 * ceil(ne / 8)) workgroups;
 * cohort order, (n_steps * ne / 64 + lead + lag) * 144 with lead / lag as clamped (auv_set_multi_order).  A call past either is
 * refused with AUV_EINVAL before anything is launched or any step number is spent.                                    */
int auv_step_multi(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev,
                   int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev);

/* auv_step_multi with EVERY step's outputs kept: n_steps consecutive step() calls (environment.py:325-384) of every slice in one launch
 * per slice, step k of the call writing
 *     its observation rows to  obs_rec    + k * N * obs_dim      [n_steps][N][obs_dim] f32   (may be NULL: no observation record)
 *     its rewards to           reward_rec + k * N                [n_steps][N] f32            (required)
 *     its done flags to        done_rec   + k * N                [n_steps][N] u8             (required)
 * with N the handle's environments -- what n_steps one-step calls hand their caller, row for row and bit for bit (tests/
 * test_gpu_multi_record.py).  An episode that ends inside the launch leaves, in the row of the step that ended it, the terminal
 * reward, done = 1 and (auto-reset) the NEW episode's first observation: the VecEnv convention.  A caller that fills a longer rollout
 * buffer in pieces passes pointers already offset to its row.  The launch is k_step_multi's (csrc/k_step_fused.hip, k_step_record:
 * the same roles, carry records, marks, workgroup order and polls; only the base address of the three outputs depends on the step),
 * so state, counters, episode log and every readable field are what auv_step_multi with the same arguments leaves.  obs_dev /
 * reward_dev / done_dev hold the LAST step's values afterwards: a small copy kernel behind the launch, on the slice's stream, copies
 * the record's last row of the slice into them (with obs_rec == NULL the launch itself writes every step's observation to obs_dev,
 * as auv_step_multi does, and only reward and done are copied).  Preconditions and refusals are auv_step_multi's, checked before
 * anything launches or any step number is spent, plus AUV_EINVAL for a NULL reward_rec / done_rec and for an obs_rec that is not
 * 8-byte aligned when obs_dim is even (the navigation features of a row are stored as float pairs then; 4 bytes when it is odd).
 * Workgroup order: auv_set_multi_order.  Eager only.  After a hand-over time-out (auv_health) the rows of steps that were not reached
 * are left as the caller passed them, and nothing is copied into obs_dev / reward_dev / done_dev; recovery is the usual one.      */
int auv_step_multi_record(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev,
                          int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev, float* reward_dev,
                          uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec);

/* CLOSED-LOOP launch of several steps: n_steps consecutive step() calls (environment.py:292-347) of every slice in one launch per
 * slice, the action of every step chosen INSIDE the launch by an affine feedback law of the observation the step before it left.
 * Per environment e there is a gain row G[e][2][8] in fp64 (gains_dev).  For output j in {0 thrust, 1 rudder} of step t:
 *     x_c = OBS64[e][c] for c = 0..5: the six navigation columns as step t - 1 left them (after an auto-reset the new episode's
 *           reset row; for the launch's first step what the arrays hold),
 *     x_6 = 1.0,
 *     x_7 = component j of the ring's action in slot (first_slot + t) % n_slots, converted to fp64 as every step converts its
 *           action; 0.0 when no ring is passed (actions_dev == NULL),
 *     p_c = G[e][j][c] * x_c,
 *     a_j = ((p_0 + p_1) + (p_2 + p_3)) + ((p_4 + p_5) + (p_6 + p_7)),
 * in fp64 with FMA contraction off and exactly this association.  `a` is the step's action: the NaN rule and the clip to the action
 * range stay where they are, in the dynamics (vessel.py:226-247).  Column 7 = 1 makes the law a residual on an open-loop sequence
 * (exploration noise, CEM candidates around a controller), column 7 = 0 pure feedback; columns 0..6 = 0 with column 7 = 1 reproduce
 * auv_step_multi_record bit for bit.  Host mirror: gym_auv_amd/feedback.py, affine_action; the launch is bit for bit n_steps
 * one-step calls fed by it (tests/test_gpu_feedback.py).  The finish wave of step t forms the action of step t + 1 and hands it to that
 * step's dynamics wave in three further words of the carry record, checksummed like the state (csrc/k_step_fused.hip,
 * k_step_feedback); everything else is auv_step_multi_record's launch.
 *     obs_rec / reward_rec / done_rec   as auv_step_multi_record's, but EACH may be NULL: no record of that output (its every step
 *                                       is then written to obs_dev / reward_dev / done_dev, which hold the last step's values
 *                                       afterwards either way)
 *     act_rec                           [n_steps][N][2] f64 or NULL: `a` of every step, before the NaN rule and the clip
 * Preconditions are auv_step_multi_record's -- the one-launch shape for every slice, at most 64 obstacles per world, no fresh world
 * per reset, the dispatch limit, obs_rec's alignment -- plus a non-NULL, 8-byte aligned gains_dev and n_slots >= 1 when a ring is
 * given; every refusal is AUV_EINVAL, before anything launches or any step number is spent.  Eager only.                       */
int auv_step_feedback(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const double* gains_dev,
                      const void* actions_dev, int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps, float* obs_dev,
                      float* reward_dev, uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec, double* act_rec);

/* auv_step_feedback with LiDAR SECTOR inputs in the law: n_steps consecutive step() calls (environment.py:292-347) in one launch per
 * slice, the action of every step formed inside the launch from the navigation columns AND the closeness columns of the observation
 * the step before it left (Vessel.perceive's row, sensor.py:140-159; the sectors are the reference's own partition of the beams,
 * utils/sector_partitioning.py:4-9, sensor.py:197, unless the caller gives another).  The OBS64 row holds L closeness columns from
 * column 6 on: L = n_sensors, or the number of sectors in the feasibility-pooled configuration.  sector_bounds_host is a table
 * b[0 .. n_sectors], 1 <= n_sectors <= 16, 0 <= b[0] <= b[1] <= ... <= b[n_sectors] <= L, read during the call (host memory):
 *     z_k = max of OBS64[e][6 + i] over b[k] <= i < b[k+1]  (from the range's first element on with m = v > m ? v : m; +0.0 for an
 *           empty range) for k < n_sectors, +0.0 for n_sectors <= k < 16,
 *     q_k = H[e][j][k] * z_k with the sector gains H[e][2][16] in fp64 (sector_gains_dev),
 *     u_j = ((q_0 + q_1) + (q_2 + q_3)) + ((q_4 + q_5) + (q_6 + q_7)),   w_j = the same association over q_8 .. q_15,
 *     a_j = s_j + (u_j + w_j),   s_j = auv_step_feedback's eight-term sum, unchanged,
 * fp64, FMA contraction off, exactly this association.  Host mirror: gym_auv_amd/feedback.py, sector_action; the launch is bit for
 * bit n_steps one-step calls fed by it (tests/test_gpu_feedback_sectors.py).  The finish wave of step t reads the closeness columns
 * where it reads columns 0..5 -- behind the sweep's pair word and its own store drain -- lane c of a group of eight taking the
 * maxima of sectors c and 8 + c (csrc/k_step_fused.hip, k_step_sector_feedback); the hand-over of the action is
 * auv_step_feedback's, and so is every other argument.
 * Preconditions are auv_step_feedback's plus: the LiDAR on (use_lidar), a non-NULL, 8-byte aligned sector_gains_dev, a non-NULL
 * sector_bounds_host, n_sectors and the bounds as above; every refusal is AUV_EINVAL, before anything launches or any step number
 * is spent.  Eager only.                                                                                                        */
int auv_step_feedback_sectors(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const double* gains_dev,
                              const void* actions_dev, int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps,
                              float* obs_dev, float* reward_dev, uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec,
                              double* act_rec, const double* sector_gains_dev, const int32_t* sector_bounds_host, int32_t n_sectors);

/* auv_step_feedback_sectors with ONE HIDDEN LAYER in the law: n_steps consecutive step() calls (environment.py:292-347) in one launch
 * per slice, the action of every step formed inside the launch from the navigation columns, the ring's action and the sector inputs
 * (Vessel.perceive's row, sensor.py:140-159; utils/sector_partitioning.py:4-9, sensor.py:197) through 16 hidden units per
 * environment -- the smallest law that can say "steer away only when something is close on that side".  The hidden layer's inputs,
 * the same for both outputs:
 *     v_0..5  = x_0..5 of auv_step_feedback, with the same source rules at step 0 and after an auto-reset,
 *     v_6, v_7 = the two components of the ring's action for the step, converted as every step converts its action (no ring: 0.0),
 *     v_8..23 = z_0..15 of auv_step_feedback_sectors (the same bounds table, the same maxima).
 * Hidden unit h has weights w_h[0..23] and a bias b_h:
 *     s = b_h;  for i = 0, 1, ..., 23 in this order  s = s + (w_h[i] * v_i)      (every product and every sum rounded once),
 *     activation 0 (relu):       y_h = s > 0.0 ? s : +0.0                         (a NaN gives +0.0),
 *     activation 1 (hard tanh):  y_h = s > 1.0 ? 1.0 : (s < -1.0 ? -1.0 : s)      (a NaN passes on to the dynamics' NaN rule),
 * and with output weights V[2][16], r_k = V[j][k] * y_k:
 *     ha_j = ((r_0 + r_1) + (r_2 + r_3)) + ((r_4 + r_5) + (r_6 + r_7)),   hb_j = the same association over r_8 .. r_15,
 *     a_j = (s_j + (u_j + w_j)) + (ha_j + hb_j),   the first bracket auv_step_feedback_sectors' result, unchanged,
 * fp64, FMA contraction off, exactly this association.  The affine part stays as a skip connection: V = 0 gives the sector launch's
 * values; smaller nets are rows of zeros.  hidden_dev is one fp64 block [N][16][28]: row h = (w_h[0..23], b_h, V[0][h], V[1][h], one
 * pad word), 224 bytes.  Host mirror: gym_auv_amd/feedback.py, hidden_action (pack_hidden makes the block); the launch is bit for bit
 * n_steps one-step calls fed by it (tests/test_gpu_feedback_hidden.py).  Lane c of a group of eight owns units c and 8 + c and takes
 * the inputs from its group by DPP moves (csrc/k_step_fused.hip, fb_hidden, k_step_hidden_feedback); the hand-over of the action is
 * auv_step_feedback's, and so is every other argument.
 * Preconditions are auv_step_feedback_sectors' plus: a non-NULL, 16-byte aligned hidden_dev and activation 0 or 1; every refusal is
 * AUV_EINVAL, before anything launches or any step number is spent.  Eager only.                                                */
int auv_step_feedback_hidden(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const double* gains_dev,
                             const void* actions_dev, int32_t action_dtype, int32_t n_slots, int32_t first_slot, int32_t n_steps,
                             float* obs_dev, float* reward_dev, uint8_t* done_dev, float* obs_rec, float* reward_rec, uint8_t* done_rec,
                             double* act_rec, const double* sector_gains_dev, const int32_t* sector_bounds_host, int32_t n_sectors,
                             const double* hidden_dev, int32_t activation);

/* Workgroup order of auv_step_multi's launches (same results either way).  order 0: step-major (all of step t, role by role, then
 * step t + 1).  order 1 (default): cohort-pipelined -- cohorts of 64 environments; the sweeps of a cohort-step are dispatched `lead`
 * cohort positions behind its dynamics and its finish waves `lag` positions behind the sweeps, so a wave finds its inputs instead of
 * holding a wave slot while it polls; lead + lag are cut down to (cohorts of the slice) - 1, which keeps every producer ahead of its
 * consumer in dispatch order; slices that are not a multiple of 64 environments, or of fewer than 3 cohorts, use order 0.
 * Defaults: order 1, lead 16, lag 30 (measured at 4096 x 180: tools/lead_lag_grid.sh).                                           */
int auv_set_multi_order(auv_handle_t* h, int32_t order, int32_t lead, int32_t lag);
/* How many obstacle boundary segments the LiDAR wave stages in LDS per batch of its pair sweep (sensor.py:140-159 is evaluated per
 * (segment, ray) pair; a crowded environment takes several batches).  Picked when a bank is loaded or generated: the largest of
 * 32 .. 96 that leaves the one-launch step its best occupancy -- every role of that launch is charged the sweep's LDS slice, so at
 * 256 beams + 47 obstacles + 17 movers a 96-segment stage (12.7 KB) means 12 waves per CU, a 34-segment one 16.  Results do not
 * depend on it (tested bit for bit).  segments = 0: only report; 32 .. 96 (even): override (a new bank picks again; graphs captured
 * before keep the stage they were captured with).  *out_segments (may be NULL) <- the value in force.              */
int auv_lidar_stage(auv_handle_t* h, int32_t segments, int32_t* out_segments);

/* VecEnv.step_async / step_wait (scripts/run.py:293-296: SubprocVecEnv sends the actions to its workers and collects their
 * results) with the ordering between the caller's stream and the chains done INSIDE the library, one call each:
 *   auv_step_async  the actions were produced on `caller_stream`; slice i is stepped on streams[i] behind them.  A slice whose
 *                   stream IS caller_stream is simply enqueued there (stream order, no hand-over at all).
 *   auv_step_wait   work enqueued on `caller_stream` after this call sees obs / reward / done of every slice.
 * Neither call blocks the host.  `rendezvous` picks the mechanism for the slices on other streams:
 *   AUV_RDV_EVENTS  one hipEventRecord behind the actions + one hipStreamWaitEvent per chain; one record + wait per chain back.
 *   AUV_RDV_DEVICE  one-wave kernels and two words in device memory: the caller's stream publishes "actions of step t ready",
 *                   a one-wave kernel in front of each chain's launch polls for it (bounded), a one-wave kernel behind it counts
 *                   the chain off, ONE polling kernel on the caller's stream waits for all of them (csrc/k_step_fused.hip:
 *                   k_rdv_*).  Every waiter waits for something submitted before it.  Needs streams whose kernels really
 *                   execute side by side: where dispatches are serialised -- a counter-collecting profiler -- a polling
 *                   kernel would sit in front of the kernel it waits for.  So (i) the first call on a set of streams runs a
 *                   TRIAL of the pattern with nothing at stake (50 ms limit; synchronises those streams once): if it runs out,
 *                   and whenever a slice is not stepped in the one-launch shape, the handle uses AUV_RDV_EVENTS instead, for
 *                   good (auv_health [7]); (ii) a real wait that runs out (auv_set_rendezvous_limit, default 10 s: raise it if
 *                   the caller's stream can be busy for longer between two steps) is reported by the next call (AUV_ESTATE,
 *                   once), and a chain whose gate ran out does NOT step: the gate raises the abort flag and the launch behind
 *                   it -- and every launch queued behind that -- hands out ABORT packets (environments untouched).
 *   AUV_RDV_CP      the same words written and awaited by the command processors (hipStreamWriteValue64 / WaitValue64).
 * Results are bit-identical to auv_step.  What a full rendezvous per step costs, and why K chains cannot beat ONE launch
 * when every step waits for all of them, is in DESIGN.md section 4.                                                      */
enum { AUV_RDV_EVENTS = 0, AUV_RDV_DEVICE = 1, AUV_RDV_CP = 2 };
int auv_step_async(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const void* actions_dev,
                   int32_t action_dtype, float* obs_dev, float* reward_dev, uint8_t* done_dev, void* caller_stream,
                   int32_t rendezvous);
int auv_step_wait(auv_handle_t* h, void* caller_stream);
int auv_set_rendezvous_limit(auv_handle_t* h, double seconds);

/* The same with every sub-batch's launch stamped with its own start / stop HIP event on ITS stream (the kernel's own
 * duration while the other chains run beside it, as a kernel trace reports it): out_ms[n_slices].  Waits for the
 * step's launches (not for earlier work on other streams).  One-launch shape only.                            */
int auv_step_pipelined_timed(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                             const void* actions_dev, int32_t action_dtype, float* obs_dev, float* reward_dev,
                             uint8_t* done_dev, float* out_ms);

/* Episode log: what the reference appends to env.history when an episode ends (save_latest_episode,
 * environment.py:466-489), for all environments of the batch, in completion order.  Row = 8 doubles: environment,
 * return (cumulative reward), timesteps, collision, reached_goal, progress, mean |cross-track error| in metres over the
 * episode's steps (_save_latest_step, environment.py:460-464), world index.  Copies rows [first, first + max_rows) of
 * the log (as far as they exist) to dst_dev on `stream` and returns the number of episodes logged so far in
 * *out_total (this read synchronises `stream`; the count is 64-bit and never wraps).  The device keeps the newest
 * 2^k >= max(65536, 4 N) rows.  A reader that has fallen further behind than that is not refused: the copy starts at the
 * oldest row still held, *out_first (nullable) tells which row that is (= first when nothing was lost; *out_first - first
 * rows were overwritten before they were read), and the caller carries on from *out_first + rows copied.  The log
 * restarts (count 0) whenever a bank is loaded or generated.                                                        */
int auv_episode_log(auv_handle_t* h, double* dst_dev, int64_t max_rows, int64_t first, int64_t* out_total,
                    int64_t* out_first, void* stream);

/* Do kernels on these two streams run side by side?  HIP multiplexes streams onto a few hardware queues (four by
 * default); two streams that land on the same one run their kernels one after the other, and sub-batch chains on them
 * do not overlap.  Launches a 300 us do-nothing wave on each and reports (wall time until both have ended) / 300 us:
 * about 1 when they overlap, about 2 when they do not.  Synchronises both streams.  For choosing the streams of
 * auv_step_pipelined (BatchedAuvEnv.set_sub_batches does).                                                        */
int auv_streams_overlap(auv_handle_t* h, void* stream_a, void* stream_b, float* out_ratio);

/* The three kernels of step(), individually launchable (per-kernel parity tests):        */
/* K1  Vessel.step: clip -> RKF45 of the 3-DOF model -> wrap psi.  (vessel.py:226-247,561-578) */
int auv_step_dynamics(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, void* stream);
/* K2  _update (movers) + Vessel.perceive: LiDAR sweep.   (environment.py:386-392, vessel.py:249-368)
 *     advance_movers = 0 skips the mover update (observe() at reset time).                 */
int auv_lidar(auv_handle_t* h, int32_t advance_movers, void* stream);
/* K3  Vessel.navigate + rewarder.calculate + _isdone + observation assembly.
 *     (vessel.py:461-541, rewarder.py:78-241, environment.py:263-280, 325-347, 375-384)
 *     mode 0: full; 1: navigation + observation only (reset path), no reward/done;
 *     2: reward/done only, from NAV64 / INFO64 / LIDAR_D / COLLISION as they stand (test hook). */
int auv_nav_reward(auv_handle_t* h, int32_t mode, float* obs_dev, float* reward_dev,
                   uint8_t* done_dev, void* stream);

/* Stream-ordered copies between handle-owned buffers and caller DEVICE buffers.           */
int auv_read(auv_handle_t* h, int32_t field, void* dst_dev, size_t bytes, void* stream);
int auv_write(auv_handle_t* h, int32_t field, const void* src_dev, size_t bytes, void* stream);
/* Size in bytes of a field for this handle (0 if unknown).                                 */
size_t auv_field_bytes(const auv_handle_t* h, int32_t field);

/* Capture one auv_step into a hipGraph bound to the given I/O pointers and replay it.     */
int auv_graph_capture(auv_handle_t* h, const void* actions_dev, int32_t action_dtype,
                      float* obs_dev, float* reward_dev, uint8_t* done_dev, void* stream);
int auv_graph_launch(auv_handle_t* h, void* stream);
/* The same with n_steps consecutive steps in ONE graph, so that the fixed cost of a replay is paid once
 * per n_steps steps (open-loop stretches: the action ring feeds step k of the replay from slot
 * (position + k) % n_slots; without a ring every step reads the same buffer).  obs / reward / done
 * hold the LAST step's values after a replay; per-env episode statistics keep accumulating.          */
int auv_graph_capture_steps(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, float* obs_dev,
                            float* reward_dev, uint8_t* done_dev, int32_t n_steps, void* stream);

/* Captured CHAINS (BASELINE configs[4] names a hipGraph-captured step): n_steps consecutive steps of every slice in the
 * one-launch shape, each slice a chain with a position of its own in the action ring (so the chains may drift apart like
 * eager chains do; all of them read the one ring of auv_set_action_ring).
 *   one_graph = 0   one LINEAR graph per slice; auv_graph_launch_chains replays slice i's graph on streams[i] -- which
 *                   hardware queue a chain runs on stays the caller's choice (auv_streams_overlap), as for eager chains.
 *   one_graph = 1   ONE graph whose n_slices branches are the chains (fork behind the root, join at the end), replayed
 *                   with auv_graph_launch; the runtime places the branches.
 * obs / reward / done hold the last step's values after a replay.                                                    */
/* (A slice stepped in the three-launch shape -- set_step_mode, no LiDAR, hand-overs disabled -- is captured in that shape and
 * advances its own ring position just the same.)                                                                      */
int auv_graph_capture_chains(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, const void* actions_dev,
                             int32_t action_dtype, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps,
                             int32_t one_graph);
int auv_graph_launch_chains(auv_handle_t* h, int32_t n_slices, void* const* streams);

/* Action ring (captured graphs only): after this call `actions_dev` of auv_graph_capture is a ring
 * of n_slots consecutive [N][2] buffers; replayed step k reads slot k % n_slots (the position lives
 * on the device and is advanced by the step itself), so a policy can fill slot k+1 while step k
 * runs and a replayed hipGraph needs no per-step argument update.  n_slots = 1 restores the plain
 * buffer.  Invalidates a captured graph.  EAGER auv_step / auv_step_timed never use the ring: they
 * read `actions_dev` as one plain [N][2] buffer and leave the ring position alone (a caller that
 * launches eagerly passes whatever pointer it likes per step).  Loading or generating a bank
 * resets the ring to one slot.                                                                */
int auv_set_action_ring(auv_handle_t* h, int32_t n_slots);

/* How auv_step / auv_step_slice / auv_graph_capture run a step (same results, bit for bit):
 *   AUV_STEP_AUTO (default)          AUV_STEP_ONE_LAUNCH for launches of fewer than 65536 environments,
 *                                    AUV_STEP_SIDE_BY_SIDE from there on (beyond the sizes the one launch was
 *                                    measured ahead at).
 *   AUV_STEP_ONE_LAUNCH              the whole step in ONE launch of one-wave workgroups with four roles: the
 *                                    first n / 8 integrate the dynamics (K1, eight environments per wave), the
 *                                    next n sweep the LiDAR of one environment each (K2), the next n search the
 *                                    nearest point of one environment's path each (the wide part of K3-nav), the
 *                                    last n / 8 -- eight environments per wave -- evaluate the navigation's scalar
 *                                    tail and run reward / done / auto-reset (K3-reward).  The roles hand their
 *                                    results on inside the launch through per-environment words and checksummed
 *                                    64-byte records stored and loaded coherently (csrc/k_step_fused.hip:
 *                                    k_step_roles, roles_finish_wave); waves that need a result poll for it, bounded.
 *   AUV_STEP_SIDE_BY_SIDE            K1 -> [K2 and K3-nav side by side in one launch] -> K3-reward: nothing is
 *                                    handed over inside a launch.  Inside a captured graph of several steps
 *                                    K3-reward of step t and K1 of step t + 1 share a launch (also what a graph
 *                                    of several steps captured in the modes above uses: it replays faster).
 * The in-launch hand-overs of ONE_LAUNCH assume that the workgroups of a launch are dispatched in index
 * order (a polling wave's producer has a smaller index; true on gfx950, not promised by HIP).  Every bank load
 * therefore runs a probe launch of the same structure (more one-wave workgroups than the chip has slots, three
 * generations polling each other); if any of its polls runs out, and whenever the LiDAR is off, the handle steps in
 * AUV_STEP_SIDE_BY_SIDE whatever mode is set.  Should a poll of a real step ever run out (bounded: seconds), the
 * wave marks the environments it leaves unfinished and raises a device-wide flag on which the launches queued behind
 * it do nothing (their dynamics role hands out ABORT packets); the NEXT call on the handle returns AUV_ESTATE once,
 * having reset exactly the marked environments (auv_health tells which launch reported and how many), cleared the
 * hand-over words and switched the handle to AUV_STEP_SIDE_BY_SIDE for good; later calls succeed.  A step
 * replayed from a captured graph (hipGraphLaunch, or a torch CUDAGraph around auv_step) is not checked per replay:
 * poll auv_health() once per rollout there.
 * (Removed in round 3, measured slower: the whole step as one kernel, [K1 + K3-nav] -> [K2 + K3-reward], K3-nav
 * forked onto a second stream, and K1 -> [K2 | K3-nav + K3-reward]; their enum values 1 .. 4 are rejected.)      */
enum { AUV_STEP_SIDE_BY_SIDE = 0, AUV_STEP_ONE_LAUNCH = 5, AUV_STEP_AUTO = 6 };
int auv_set_step_mode(auv_handle_t* h, int32_t mode);
/* The shape a launch of n_envs_per_launch environments (<= 0: the whole batch) is really stepped in: AUV_STEP_*. */
int auv_effective_step_mode(auv_handle_t* h, int32_t n_envs_per_launch);
/* out8: [0] 1 = in-launch hand-overs in use, [1] polls of the last dispatch-order probe that ran out (-1: no bank yet),
 *       [2] hand-over time-outs over the life of the handle, [3] 1 = a time-out is pending (the next step call
 *       will recover and return AUV_ESTATE), [4] / [5] e0 / ne of the launch that reported the last time-out (-1: none),
 *       [6] environments the last recovery reset, [7] 0 while AUV_RDV_DEVICE is in use, else the number of rendezvous
 *       waits (trial included) that ran out -- events from then on.  Reads host memory only: no synchronisation.
 * A recovery writes the reset observation of the environments it resets into OBS64 and into the obs buffer of the CALL THAT
 * RECOVERS (if that call has one) -- never through a pointer remembered from an earlier call.                     */
int auv_health(auv_handle_t* h, int32_t* out8);
/* The dispatch-order probe on the streams production uses: one probe launch per stream, all in flight together, a foreign
 * kernel behind each, two rounds (BatchedAuvEnv.set_sub_batches runs it on the chain streams it has chosen).  Updates
 * what auv_health reports in [0] / [1]; a probe that fails is not an error -- the handle then steps in the
 * three-launch shape.  Synchronises the device.                                                                   */
int auv_probe_streams(auv_handle_t* h, int32_t n_streams, void* const* streams);

/* One step with every dispatch stamped with its own start / stop HIP event on `stream` (the kernel's
 * own duration, as a kernel trace reports it).  out_ms[0..3] by effective mode:
 *   AUV_STEP_ONE_LAUNCH    the one launch, 0, 0, whole step
 *   AUV_STEP_SIDE_BY_SIDE  K1, [K2 + K3-nav], K3-reward, whole step. */
int auv_step_timed(auv_handle_t* h, const void* actions_dev, int32_t action_dtype, float* obs_dev,
                   float* reward_dev, uint8_t* done_dev, void* stream, float* out_ms4);

/* Feasibility-pooled observations (VesselConfig.sensor_use_feasibility_pooling; the dimensionality reduction of the
 * gym-auv paper).  The observation row becomes [6 navigation features | n_sectors closenesses | (velocity channels:
 * 2 * n_sectors zeros)]: the closeness (sensor_log_transform or linear, vessel.py:88-95) of each sector's feasible distance,
 * LidarPreprocessor._feasibility_pooling (sensor.py:251-296) over sensors sector_start[k] .. sector_start[k+1]-1 with
 * opening width `width` (= vessel_width * feasibility_width_multiplier) and sensor spacing 2*pi/S -- bit for bit what
 * auv_feasibility_pooling computes on the same ranges.  Every step shape produces it (the LiDAR wave pools its own
 * ranges); the float32 rows the caller passes are 6 + c * n_sectors wide (c = obs_channels), and so is a policy's obs_dim.
 * Unchanged by pooling: the ranges (LIDAR_D), collision, both rewarders' LiDAR terms, done, info, the episode log and the
 * state -- they read the full ranges, as in the reference.  OBS64 keeps its stride (see the field).
 *   sector_start_host [n_sectors + 1] int32, host memory: strictly increasing from 0 to n_sensors (gym_auv_amd.pooling.
 *   sector_starts gives the reference's sigmoid partition).  n_sectors = 0: off (the default).  width: finite, > 0.
 * Only between auv_create and the first bank load (auv_load_worlds / auv_generate_worlds / auv_fresh_worlds_create): the
 * per-world reset rows depend on it -- later calls return AUV_ESTATE; a malformed table AUV_EINVAL.  With use_lidar = 0 the
 * call is accepted and changes nothing (the observation has no LiDAR columns).                                             */
int auv_set_obs_pooling(auv_handle_t* h, int32_t n_sectors, const int32_t* sector_start_host, double width);

/* Feasibility pooling (optional post-kernel on the current LiDAR ranges):
 * for every env and sector k (sensors sector_start[k] .. sector_start[k+1]-1) the feasible
 * distance of LidarPreprocessor._feasibility_pooling (sensor.py:251-296) with opening width
 * `width` (= vessel_width * feasibility_width_multiplier) and sensor spacing 2*pi/S.
 * sector_start_dev: [n_sectors+1] int32; out_dist_dev: [N][n_sectors] fp64 (nullable);
 * out_closeness_dev: [N][n_sectors] f32 closeness of those distances (nullable).            */
int auv_feasibility_pooling(auv_handle_t* h, const int32_t* sector_start_dev, int32_t n_sectors, double width,
                            double* out_dist_dev, float* out_closeness_dev, void* stream);

/* On-device scenario generation: build n_worlds MovingObstacles-type worlds on
 * the GPU, one workgroup per world, straight into fixed-capacity world slots, then compute their
 * reset rows and reset every environment -- the device-side replacement of
 * MovingObstacles._generate (envs/movingobstacles.py:28-95: RandomCurveThroughOrigin path with its
 * three PCHIP passes, objects/path.py:19-40,96-120; vessel start; helpers.generate_obstacle
 * placements, utils/helpers.py:5-35; VesselObstacle / CircularObstacle tables,
 * objects/obstacles.py:90-113,144-215).  Replaces any previous bank, like auv_load_worlds.
 *   draws_dev [n_worlds][n_draws] fp64 DEVICE memory, n_draws = 11 + n_moving*(3*C+2) + n_static*3*C
 *   with C = AUV_GEN_CAND: row = u_nwaypoints, u_angle, 6 waypoint jitters, start ux, uy, upsi, then
 *   per mover C x (z ~ N(0,1), u, Poisson(10)) + u_direction + u_speed, then per circle
 *   C x (z, u, Poisson(30)); u ~ U[0,1).  The unbounded rejection loop of generate_obstacle is
 *   a pool of C candidates (first accepted wins); if the whole pool is rejected (~1e-13 per obstacle)
 *   up to 56 more come from a counter-based generator keyed by the pool (gym_auv_amd/devgen.py,
 *   extra_candidate), so that no obstacle is placed on the vessel or the goal.
 *   ring_unit [65][2], nseg_by_radius [n_radius] HOST tables: unit ring of the GEOS point buffer
 *   and the number of segments Douglas-Peucker(0.3) leaves for an integer radius (4..64, power
 *   of two); needed on the first call of a given shape, ignored afterwards.
 * A second call with the same (n_worlds, n_moving, n_static) regenerates in place without
 * allocating.  Synchronous.                                                                   */
#define AUV_GEN_CAND 8
#define AUV_GEN_POLY_CAP 16384   /* polyline vertices per generated world slot (path <= 1638 m) */
int auv_generate_worlds(auv_handle_t* h, int32_t n_worlds, int32_t n_moving, int32_t n_static,
                        const double* draws_dev, int32_t n_draws, const double* ring_unit,
                        const int32_t* nseg_by_radius, int32_t n_radius);

/* Read a table of a GENERATED bank back (device-to-device copy; slot layout: world w owns
 * [w*cap, (w+1)*cap) of each table, counts in AUV_B_POLY_CNT / OBS_META).  For tests and for
 * checkpointing generated worlds.                                                              */
enum {
  AUV_B_POLY_CNT = 0,     /* [W] int32                      */
  AUV_B_POLY_XY = 1,      /* [W][AUV_GEN_POLY_CAP][2]       */
  AUV_B_POLY_CUM = 2,     /* [W][AUV_GEN_POLY_CAP]          */
  AUV_B_KNOT_S = 3,       /* [W][1000]                      */
  AUV_B_KNOT_COEF = 4,    /* [W][1000][8]                   */
  AUV_B_WORLD_SCALAR = 5, /* [W][8]                         */
  AUV_B_OBS_META = 6,     /* [W][K][4] int32                */
  AUV_B_OBS_CULL = 7,     /* [W][K][3]                      */
  AUV_B_SEG = 8,          /* [W][64*n_static][4]            */
  AUV_B_MV_PARAM = 9,     /* [W][M][4]                      */
  AUV_B_MV_INIT = 10,     /* [W][M][4]                      */
  AUV_B_MV_VTAB = 11,     /* [W][M][2]                      */
  AUV_B_CHUNK_BOUND = 12  /* [W][AUV_GEN_POLY_CAP/64][4]    */
};
size_t auv_bank_bytes(const auv_handle_t* h, int32_t table);
int auv_read_bank(auv_handle_t* h, int32_t table, void* dst_dev, size_t bytes, void* stream);

/* A FRESH WORLD ON EVERY RESET (both halves joined): the reference builds a new scenario whenever an episode
 * ends (environment.py:176-218 reset() -> _generate(); envs/movingobstacles.py:28-95).  auv_generate_worlds gives a bank that
 * auto-reset cycles through ((w + N) % W): fine for throughput, not what the reference's learner sees.  This mode does:
 *   - the bank is `depth` slots per environment (slot e + j N belongs to environment e; depth >= 2); the world of environment e's
 *     k-th episode is the world of (seed, env_index_base + e, serial k): draws from a counter-based generator on the device
 *     (k5_generate.hip: k5_draws; gym_auv_amd/devgen.py: counter_draws is the host mirror), so what an environment meets does not
 *     depend on timing, on the sub-batch chains, or on how the batch is sharded over GPUs (env_index_base = the shard's first
 *     GLOBAL environment index);
 *   - an environment whose episode ends (auto-reset, or auv_reset after it has stepped) moves to its next slot and queues the one
 *     it leaves; a refill pass -- ONE graph launch on a side stream, enqueued by the step calls themselves every `period` calls,
 *     paced in GPU time behind the first chain's stream and never waited for -- rebuilds exactly the queued slots (up to
 *     `batch_cap` per pass): tables (k5_generate), reset rows (the step's own kernels on batch_cap shadow environments nobody
 *     steps), and its last kernel makes them bindable.  No host round trip: the host may be thousands of launches ahead.
 *     A finish wave that binds a slot reads its tables with agent-scope loads in that launch (the pass may have completed
 *     while the launch was running); every later launch starts behind a kernel boundary.  Running environments are never touched.
 *   - should an episode end before its environment's next slot is ready (the pass fell behind an episode of a few steps) the
 *     environment starts over in the world it has just finished, and the event is COUNTED (auv_fresh_worlds_stats [2]); size
 *     `depth` / `period` / `batch_cap` so that the count stays 0 (bench.py --fresh-worlds reports it).
 * The episode log's `world` column then holds e + N * serial (what the world's index would be in a bank that never repeats).
 * auv_fresh_worlds_create replaces the bank like auv_generate_worlds (same ring tables; synchronous) and resets every
 * environment; auv_load_worlds / auv_generate_worlds leave the mode.  auv_reset refuses an explicit world_idx in this mode.
 *   auv_fresh_worlds_refill   the step calls that cover the whole batch (auv_step, _pipelined, _async, auv_policy_rollout, graph
 *                             launches) tick by themselves; a caller that drives slices one by one (auv_step_slice) calls this
 *                             with the chains' slices and streams.  flush != 0: synchronises those streams, then runs passes
 *                             until the queue is empty and everything is published (tests; a deterministic hand-over point).
 *   auv_fresh_worlds_stats    out8: [0] mode on, [1] worlds rebuilt, [2] episodes that re-used their world (see above), [3] slots
 *                             queued now, [4] passes enqueued, [5] passes completed, [6] depth, [7] batch_cap.  One small D2H copy.
 *   auv_fresh_worlds_draws    the draws row of (environment, serial) for n_rows pairs (HOST arrays of environment indices
 *                             relative to this handle) -> dst_dev [n_rows][n_draws]: what the host mirror rebuilds a world from.
 * (The pass's stream is a plain stream: creating one with a non-default priority halves the throughput of four sub-batch chains
 * on this stack even while it idles -- tools/side_stream_ab.sh.)                                                       */
int auv_fresh_worlds_create(auv_handle_t* h, int32_t depth, int32_t n_moving, int32_t n_static, uint64_t seed, int64_t env_index_base,
                            int32_t batch_cap, int32_t period, const double* ring_unit, const int32_t* nseg_by_radius, int32_t n_radius);
int auv_fresh_worlds_refill(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, int32_t flush);
/* The stream the refill passes run on (default: a plain stream the library creates).  This GPU runs at most FOUR kernels side by
 * side and HIP multiplexes streams onto four hardware queues (FIFO each): a pass on a stream that shares a queue with a chain
 * stalls that chain for the pass's duration, and beside four busy chains a pass takes a slot from one of them whatever its
 * queue (tools/side_queue_probe.py: 153 -> 70 / 95 M env-steps/s).  So: three chains plus a pass stream chosen to run side by
 * side with all three (auv_streams_overlap) -- what BatchedAuvEnv.set_sub_batches does in this mode.  The stream stays the
 * caller's; it must outlive the mode.                                                                              */
int auv_fresh_worlds_set_stream(auv_handle_t* h, void* stream);
/* Launches of SEVERAL steps with a fresh world on every reset.  auv_step_multi / auv_step_multi_record refuse this mode ("not with a
 * fresh world per reset") until the handle opts in here; the closed-loop entries (auv_step_feedback, _sectors, _hidden) refuse it
 * (AUV_EINVAL) unless the handle opts in with on == 2, which allows them as well as the two open-loop calls (on == 1: those two only).
 * on != 0 needs depth >= 3 (AUV_EINVAL) and the mode itself (AUV_ESTATE); auv_fresh_worlds_create switches it off again.
 * A closed-loop launch of an on == 2 handle forms the action of the step after a reset from the reset row of the slot the reset
 * actually took -- the next slot, or in a counted re-use the world just left -- and everything below holds for it unchanged.
 * What an opted-in handle does in those calls:
 *   - the steps of a launch read a bound slot's tables with plain loads and no kernel boundary in between, so a launch binds ONLY
 *     slots that were published before any kernel of its call began: every call has a number, a one-wave kernel in front of each
 *     chain's launch announces it on the device, the pass's last kernel stamps every slot it publishes with the latest number
 *     announced, and a launch of call c takes a slot only if its stamp is below c.  An environment whose next slot does not
 *     qualify starts over in the world it has just finished, COUNTED in auv_fresh_worlds_stats [2] like every re-use;
 *   - every call counts n_steps towards `period` and enqueues its pass BEHIND its launches, paced behind every chain: a slot left
 *     in call c is rebuilt beside call c + 1 and bindable from call c + 2 on (from c + 1 on where the caller synchronises in
 *     between).  depth 3 therefore sustains one reset per environment per launch and a burst of two;
 *   - auv_fresh_worlds_refill(flush) leaves every slot left so far bindable by the next call;
 *   - not on a stream that is being captured (the call's number is a launch argument).
 * One-step calls on the handle behave as before.                                                                        */
int auv_fresh_worlds_multi(auv_handle_t* h, int32_t on);
int auv_fresh_worlds_stats(auv_handle_t* h, int64_t* out8);
int auv_fresh_worlds_draws(auv_handle_t* h, const int32_t* envs_host, const int32_t* serials_host, int32_t n_rows, double* dst_dev,
                           void* stream);

/* ---- the policy in the loop (scripts/run.py:332-357: PPO2 with MlpPolicy, net_arch [256, 128, 64] for
 * policy and value function, tanh, diagonal Gaussian over the two actions) --------------------------------------------
 * auv_policy_act evaluates actor and critic for the environments [e0, e0 + ne) with ONE launch on `stream`, straight from
 * the observation rows the step has written: obs -> [256, 128, 64] tanh -> (mu[2] | value), f32 on the matrix cores
 * (v_mfma_f32_16x16x4_f32: exact f32), then in the epilogue a = mu + exp(log_std) eps (counter-based generator keyed by
 * seed, step counter, environment), log pi(a), the action mapped into the action space and written into the
 * environment's action buffer, and the transition stored at position t of the rollout:
 *   O[t] = obs, A[t] = a, LP[t] = log pi(a), V[t] = value, and -- of the step the environment completed BEFORE this
 *   call -- R[t - 1] = reward_scale * clip(reward), Dn[t - 1] = done.  A rollout row holds `ld` environments; environment e
 *   sits in column e - env_base of it (one [T][N] buffer shared by all sub-batches: ld = N, env_base = 0).
 * t lives on the device (ctr[0]; the host zeroes it before a rollout), is advanced by the launch itself, and a call
 * with t == T only stores R[T - 1] / Dn[T - 1] (the flush behind a rollout's last step); so the call can sit in a
 * captured graph.  params: auv_policy_param_floats(obs_dim) floats, 16-byte aligned -- the policy net then the value
 * net, each W1 [256][K0p] b1 [256] W2 [128][256] b2 [128] W3 [64][128] b3 [64] W4 [16][64] b4 [16], then log_std[2]
 * and two floats of padding.  A weight matrix is torch's Linear.weight [out][in], columns padded with zeros to a multiple
 * of 32 (K0p = obs_dim rounded up), the last layer's rows to 16, and stored in MFMA fragment order: element [n][k] at
 *   ((((n / 16) * (K / 32) + k / 32) * 2 + (k % 8) / 4) * 64 + ((k % 32) / 8) * 16 + n % 16) * 4 + k % 4
 * (gym_auv_amd/policy.py: FusedActorCritic.refresh does it with one permuted copy per layer).  All pointers are device
 * pointers.                                                                                                        */
typedef struct auv_policy_io {
  const float* obs;          /* [N][obs_dim]  the environment's observation buffer                          */
  const float* params;       /* packed weights (above)                                                       */
  int64_t* ctr;              /* [4] device: t, generator step counter (monotonic), scratch, -                */
  const float* reward_in;    /* [N]  the environment's reward buffer                                         */
  const uint8_t* done_in;    /* [N]  the environment's done buffer                                           */
  float* actions_out;        /* [N][2] the action buffer auv_step* reads (AUV_F32)                           */
  float* O;                  /* [T][ld][obs_dim] (nullable)                                                  */
  float* A;                  /* [T][ld][2]                                                                   */
  float* LP;                 /* [T][ld]                                                                      */
  float* V;                  /* [T][ld]                                                                      */
  float* R;                  /* [T][ld]                                                                      */
  float* Dn;                 /* [T][ld]                                                                      */
  float* mu_out;             /* [ne][2] (nullable: tests)                                                    */
  float* eps_out;            /* [ne][2] (nullable: tests)                                                    */
  uint64_t seed;
  int32_t obs_dim, T;
  int32_t ld, env_base;      /* environments per rollout row; the environment in column 0                   */
  float act_mid[2], act_half[2], clip_lo[2], clip_hi[2];   /* action = mid + half * clip(a, lo, hi)          */
  float reward_scale, reward_clip;                         /* reward_clip <= 0: no clipping                  */
  const void* params_bf16;   /* NULL: exact f32 (the default).  Else the eight weight matrices as bf16 -- policy net W1 W2
                                W3 W4, then the value net's, padded like the f32 ones, element [n][k] of a matrix at
                                (((n / 16) * (K / 32) + k / 32) * 64 + ((k % 32) / 8) * 16 + n % 16) * 8 + k % 8 -- and the
                                launch runs v_mfma_f32_16x16x32_bf16 (activations rounded to bf16 into the MFMA, f32
                                accumulation / bias / tanh): ~1e-2 on the means, NOT the reference's arithmetic; biases and
                                log_std still come from `params`.  16-byte aligned.                            */
} auv_policy_io_t;
size_t auv_policy_param_floats(int32_t obs_dim);
int auv_policy_act(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, void* stream);
/* n_steps transitions of every slice with ONE call: per step and slice the policy launch and the environment's step of
 * that slice (actions = ios[i].actions_out), back to back on streams[i]; `flush` != 0: a final policy call per slice
 * stores the last step's reward / done.  t0 / gstep0 (host arrays, one entry per slice; both or neither): the rollout
 * position and the generator's step counter of the FIRST launch of each slice -- the host then names them for every launch
 * (position t0 + k, generator step gstep0 + k) and the launches skip their count-off on io.ctr (~4 us per launch; the
 * device copies are still kept in step); NULL: the launches use and advance io.ctr like auv_policy_act.  The chains are
 * not ordered against each other or the caller's stream.                                                           */
int auv_policy_rollout(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                       const auv_policy_io_t* ios, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps,
                       int32_t flush, const int64_t* t0, const int64_t* gstep0);

/* ---- frame-stacked observations in the policy launch (what stable-baselines ships as VecFrameStack; csrc/k12_policy_stacked.hip) ----
 * auv_policy_act_stacked is auv_policy_act's exact-f32 launch on input rows of frames * obs_dim columns: columns [j * obs_dim,
 * (j + 1) * obs_dim) hold the observation of j steps ago -- j = 0 the observation buffer as it stands, NEWEST FIRST (a column
 * permutation of stable-baselines' newest-last order) -- and zeros where the episode is younger than j steps.  The same matrix chains
 * and the same epilogue: for the same row the mean and the value have the bits auv_policy_eval gives with obs_dim = frames * obs_dim,
 * and frames == 1 is auv_policy_act bit for bit (hist and stk are then not touched and may be NULL).
 *   io        as for auv_policy_act with:  obs_dim the ENVIRONMENT's;  params auv_policy_param_floats(frames * obs_dim) floats, the
 *             nets of the wider first layer;  O [T][ld][frames * obs_dim], the stacked rows;  params_bf16 NULL.
 *   hist      [N][frames][obs_dim] f32, a ring per environment, indexed by GLOBAL environment (16-byte aligned)
 *   stk       [N][2] int32 (8-byte aligned): word 0 = pos | tag << 8 -- pos the ring slot of the newest frame, tag marks the launch that
 *             stored it: (generator step mod (2^23 - 1)) + 1, in 1 .. 2^23 - 1, so the word is never negative (policy and value workgroup
 *             of one launch both need the state from BEFORE the launch, and the one that comes second recognises its own launch's tag;
 *             0: no launch) -- word 1 = age, the number of valid frames.  All zero: an empty history; zeroing word 1 of an environment
 *             empties its history.
 *   REQUIRED  consecutive act launches on the same rows must have DIFFERENT generator steps (mod 2^23 - 1).  The device counter
 *             (io.ctr[1]) and t0 / gstep0 advanced by the number of launches made -- what auv_policy_rollout's contract asks for anyway --
 *             give that.  A launch repeated with the generator step of the launch before it (a determinism check, a captured one-step
 *             rollout replayed with host counters) finds its own tag in stk and does NOT move the history: restore stk, or zero the tag
 *             bits (stk word 0 &= 255), before such a replay.
 *   a launch with t < T, per environment:  age' = min((done_in ? 0 : age) + 1, frames),  pos' = (pos + 1) mod frames;  frame j >= 1 of
 *             the row is hist[(pos' - j) mod frames] if j < age', else zeros;  then hist[pos'] = obs, stk = (pos', age').
 *   the flush launch (t == T) stores R[T - 1] / Dn[T - 1] only and leaves hist and stk alone: the next rollout's first launch sees
 *             the same obs and done_in and adds that frame exactly once.
 * Everything lives on the device: the launch can sit in a captured graph.  AUV_EINVAL, before anything is enqueued: what
 * auv_policy_act refuses; frames outside [1, AUV_MAX_FRAMES]; frames * obs_dim too wide for the kernel's LDS tile; params_bf16 set;
 * frames > 1 with hist or stk NULL or misaligned.
 * auv_policy_rollout_stacked is auv_policy_rollout's loop with that launch: the same t0 / gstep0 contract -- with gstep0[i] of a call
 * NOT equal to the generator step of the last act launch before it on that slice (REQUIRED, above) -- the same slices on their own
 * streams; every slice must have the same `frames`.
 * auv_stack_frames does the history update alone, no handle and no network: stacked rows out[ne][ldx] (ldx >= frames * obs_dim
 * floats; row j is environment e0 + j of obs, done, hist and stk) on `stream`.  done NULL: no environment is done.  advance != 0: hist
 * and stk move on as in an act launch (tag 0); advance == 0 is a PEEK -- the row the next act launch would form, nothing is stored to
 * hist or stk.  16-byte accesses where obs_dim, ldx and the bases allow, 8- or 4-byte ones otherwise.                              */
#define AUV_MAX_FRAMES 8
typedef struct auv_policy_stack {
  auv_policy_io_t io;
  float* hist;               /* [N][frames][obs_dim]                                                           */
  int32_t* stk;              /* [N][2]: pos | tag << 8, age                                                    */
  int32_t frames, reserved;
} auv_policy_stack_t;
int auv_policy_act_stacked(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_stack_t* io, void* stream);
int auv_policy_rollout_stacked(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                               const auv_policy_stack_t* ios, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps,
                               int32_t flush, const int64_t* t0, const int64_t* gstep0);
int auv_stack_frames(int32_t device, const float* obs, const uint8_t* done, float* hist, int32_t* stk, float* out, int64_t ldx,
                     int32_t e0, int32_t ne, int32_t obs_dim, int32_t frames, int32_t advance, void* stream);

/* ---- the policy outside the rollout (scripts/run.py:175, 273, 567: agent.predict(obs, deterministic=True) of the enjoy / play /
 * test modes; csrc/k9_policy_eval.hip) --------------------------------------------------------------------------------------------
 * auv_policy_eval evaluates M observation rows through the policy net, the value net, or both, with ONE launch on `stream`: no
 * environment handle, no rollout position, no counters, no sampling.  The matrix chains are those of auv_policy_act's exact-f32
 * path, so for the same row and the same `params` the mean and the value have the same bits as the rollout launch gives.
 *   rows      row j < M is X[(idx ? idx[j] : j) * ldx .. + obs_dim): ldx >= obs_dim, in floats; 4-byte alignment is enough.  idx as
 *             auv_ppo_batch::idx: an index that names a row outside X is the caller's error, it is not checked.
 *   outputs   each nullable, written for rows < M only:  mu[j][2] the policy mean;  action[j * action_ld + c] = act_mid[c] +
 *             act_half[c] * clip(mu[c], clip_lo[c], clip_hi[c]), the deterministic action (action_ld >= 2 floats: 2 writes straight
 *             into rows of an environment's [N][2] float32 action buffer);  value[j];  logp[j] = log pi(A[j] | row j) for the GIVEN
 *             actions A[M][2] (indexed by j, not through idx), the expression auv_policy_act stores in LP.
 *   nets      only the nets whose outputs are asked for are launched (value alone never reads the policy weights).
 * AUV_EINVAL, before anything is enqueued: logp without A; no output at all; obs_dim < 1 or too wide for the kernel's LDS tile;
 * ldx < obs_dim; action with action_ld < 2; M < 0; params not 16-byte or another pointer not 4-byte aligned.  M == 0 succeeds and
 * launches nothing.  Enqueued on `stream`; no synchronisation, no allocation.  All pointers except `ev` are device pointers.      */
typedef struct auv_policy_eval {
  const float* params;       /* the layout of auv_policy_io::params (auv_policy_param_floats(obs_dim) floats)   */
  const float* X;            /* observation rows, row stride ldx floats                                         */
  const int64_t* idx;        /* [M] rows of X to evaluate; NULL: rows 0 .. M - 1                                */
  const float* A;            /* [M][2] actions whose log-probability is asked for (needed with logp)            */
  float* mu;                 /* [M][2]        (nullable)                                                        */
  float* action;             /* [M][action_ld] (nullable)                                                       */
  float* value;              /* [M]           (nullable)                                                        */
  float* logp;               /* [M]           (nullable)                                                        */
  int64_t ldx;
  int32_t action_ld, obs_dim, M;
  float act_mid[2], act_half[2], clip_lo[2], clip_hi[2];   /* action = mid + half * clip(mu, lo, hi)          */
} auv_policy_eval_t;
int auv_policy_eval(int32_t device, const auv_policy_eval_t* ev, void* stream);

/* ---- other hidden widths than [256, 128, 64] in the fused forward launches ------------------------------------------------------
 * The launches above evaluate obs -> 256 -> 128 -> 64 -> out, the reference's net (scripts/run.py:332-357).  The *_arch entries take
 * the three hidden widths beside the same argument structs and evaluate obs -> h1 -> h2 -> h3 -> out: three tanh layers, the same
 * actor / critic shape, exact f32, outputs padded to one n-tile -- every word of the entries above holds, with the packed layout of
 * auv_policy_io::params read with (h1, h2, h3) in the place of (256, 128, 64): auv_policy_param_floats_arch(obs_dim, arch) floats,
 *   2 * (h1 * K0p + h1 + h2 * h1 + h2 + h3 * h2 + h3 + 16 * h3 + 16) + 4,   K0p = obs_dim rounded up to a multiple of 32.
 * A CLOSED LIST of triples is compiled in (csrc/auv_policy_mfma.h, POL_ARCH_LIST):
 *   (256, 128, 64)  (128, 128, 64)  (128, 64, 64)  (64, 64, 64)
 * (256, 128, 64) through an _arch entry runs the very kernels of the entry without the suffix.  AUV_EINVAL, before anything is
 * enqueued, beside what the plain entries refuse: arch NULL; a triple outside the list (it is never rounded to a listed one;
 * auv_policy_param_floats_arch then returns 0); params_bf16 set with another triple than (256, 128, 64).  The population launches
 * (auv_population_*_arch) and the fused update (auv_ppo_create_arch) take the same list, both below.                             */
typedef struct auv_policy_arch {
  int32_t h1, h2, h3;
} auv_policy_arch_t;
size_t auv_policy_param_floats_arch(int32_t obs_dim, const auv_policy_arch_t* arch);
int auv_policy_act_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, const auv_policy_arch_t* arch, void* stream);
int auv_policy_rollout_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                            const auv_policy_io_t* ios, const auv_policy_arch_t* arch, float* obs_dev, float* reward_dev,
                            uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0);
int auv_policy_act_stacked_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_stack_t* io, const auv_policy_arch_t* arch,
                                void* stream);
int auv_policy_rollout_stacked_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                                    const auv_policy_stack_t* ios, const auv_policy_arch_t* arch, float* obs_dev, float* reward_dev,
                                    uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0);
int auv_policy_eval_arch(int32_t device, const auv_policy_eval_t* ev, const auv_policy_arch_t* arch, void* stream);

/* ---- a tanh-squashed Gaussian policy (what stable-baselines3 calls squash_output; csrc/k17_policy_squash.hip) ---------------------
 * The launches above hand the environment act_mid + act_half * clamp(a, clip_lo, clip_hi) of the sample a: a box the Gaussian's
 * entropy does not see.  The *_squash entries hand it
 *     act_mid + act_half * tanh(u),   u = mu + sigma eps   (the deterministic action of the evaluation: u = mu)
 * and read neither clip_lo nor clip_hi.  EVERYTHING ELSE IS THE PLAIN ENTRY'S, BIT FOR BIT, for the same weights, seed and step: the
 * stored action A is u itself, LP the Gaussian log-density of u (the PPO ratio needs no Jacobian: it cancels), V, R, Dn, O, mu_out,
 * eps_out, the counters and their hand-over; the evaluation's mu, value and logp, which takes PRE-SQUASH actions (rows of A).  Exact
 * f32 only, at every triple of the list.  tanh is (1 - t) / (1 + t), t = exp(-2 |u|), with u's sign: odd bit for bit, exactly +-1 from
 * |u| = 20 on (so the action is exactly act_mid +- act_half there), never NaN for a finite u.  AUV_EINVAL beside what the plain
 * entries refuse: params_bf16 set.  The update that goes with it: auv_ppo_grad_squash, below.                                       */
int auv_policy_act_squash(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, void* stream);
int auv_policy_act_squash_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_io_t* io, const auv_policy_arch_t* arch,
                               void* stream);
int auv_policy_rollout_squash(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_io_t* ios,
                              float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0,
                              const int64_t* gstep0);
int auv_policy_rollout_squash_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                                   const auv_policy_io_t* ios, const auv_policy_arch_t* arch, float* obs_dev, float* reward_dev,
                                   uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0);
int auv_policy_eval_squash(int32_t device, const auv_policy_eval_t* ev, void* stream);
int auv_policy_eval_squash_arch(int32_t device, const auv_policy_eval_t* ev, const auv_policy_arch_t* arch, void* stream);

/* ---- running observation and reward normalisation (what stable-baselines ships as VecNormalize; csrc/k16_policy_norm.hip) ----------
 * DEVIATION from stable-baselines: it updates its statistics at every step_wait, before normalising that step's batch.  Here the
 * statistics are FROZEN while launches run and FOLDED between rollouts: a per-step update would be a reduction over all environments
 * between the environment's launch and the policy launch of every step -- a barrier across chains that are not ordered against each
 * other, and a result that depends on their timing.  So the first rollout runs on the initial table (mean 0, variance 1), every later
 * one on the statistics of all rollouts before it, and a rollout's rewards are scaled by a deviation that already holds ALL of that
 * rollout's returns (stable-baselines: the returns up to that step).  Initial state, stable-baselines' RunningMeanStd: mean 0, variance
 * 1 (M2 = count), count 1e-4.
 *
 * auv_policy_act_norm is auv_policy_act's exact-f32 launch with one step between the tile's load and the matrix chains:
 *   x' = min(max((x - mean[c]) * inv_std[c], -clip_obs), clip_obs)      three separately rounded f32 operations and the clamp
 * The nets see x'; O[t] holds x' -- the rows the fused update gathers, so nothing behind the launch changes -- and for the same row the
 * mean and the value have the bits auv_policy_eval gives on auv_norm_rows' output.
 *   table     [obs_dim][2] f32 = (mean, inv_std) per column, 8-byte aligned; nobody may write it while launches that read it run
 *   part      [T * part_ld][2][obs_dim] f32: per launch position t and 16-row tile, the moments of the tile's RAW rows -- [0] the mean
 *             m = s / rows of the sequential f32 sum s over rows 0 .. rows - 1, [1] M2 = the sequential sum of (x_r - m)^2, every
 *             operation separately rounded.  The tile `i` of a launch on [e0, e0 + ne) at position t writes slot t * part_ld +
 *             part_base + i: part_base is the prefix sum of ceil(ne / 16) over the slices in front, part_ld the sum over all.
 *   pcnt      [T * part_ld] int32: the rows of that tile (16, or fewer in a slice's last tile); 0 = an empty slot, skipped by the fold
 *   the flush launch (t == T) stores R[T - 1] / Dn[T - 1] only, as auv_policy_act's does.
 * Only the policy workgroup of a tile stores (O, part, pcnt); the value workgroup normalises its own copy of the tile.  Rewards are
 * stored RAW, as by auv_policy_act (reward_scale and reward_clip of io apply as they do there).
 * AUV_EINVAL, before anything is enqueued: what auv_policy_act refuses (obs_dim too wide for the LDS tile among it); table NULL or
 * not 8-byte aligned; part or pcnt NULL or not 4-byte aligned; params_bf16 set; clip_obs not > 0; part_base < 0 or part_base +
 * ceil(ne / 16) > part_ld; with _arch: arch NULL or a triple outside the list.  Frame stacking is not combined with it: there is no
 * stacked form of this struct.
 * auv_policy_rollout_norm is auv_policy_rollout's loop with that launch: the same t0 / gstep0 contract, the same slices on their own
 * streams.
 *
 * auv_norm_rows: the same expression on M arbitrary rows, no handle and no network: out[j * ldo + c] = x'(X[(idx ? idx[j] : j) * ldx
 * + c]) for c < obs_dim, on `stream` -- what goes in front of auv_policy_eval outside a rollout; the bits the act launch stores in O.
 * AUV_EINVAL: device < 0; obs_dim outside [1, 16384]; M < 0; X, out or table NULL; table not 8-byte, idx not 8-byte, X or out not
 * 4-byte aligned; ldx or ldo < obs_dim; clip_obs not > 0.  M == 0 succeeds and launches nothing.
 *
 * auv_norm_fold merges the n_slots partials of (part, pcnt) into the running moments and rewrites the table; one launch on `stream`.
 *   mom       [obs_dim][3] f64 = (count, mean, M2) per column
 *   merge     Chan's pairwise formula in fp64, every operation separately rounded; merge(a, b) with tot = a.n + b.n, delta = b.mean -
 *             a.mean:  mean = a.mean + (delta * b.n) / tot,  M2 = (a.M2 + b.M2) + (((delta * delta) * a.n) * b.n) / tot;  b.n == 0
 *             gives a, a.n == 0 gives b.
 *   order     one wave per column: lane l merges the slots l, l + 64, ... in that order, each as b, skipping pcnt <= 0; the 64 lane
 *             results merge as a tree -- for o = 32, 16, 8, 4, 2, 1: lane l < o becomes merge(lane l, lane l + o); the result merges
 *             into the running moments as b.  No atomics: a rerun from the same state is bit-identical.
 *   table     mean = (float)mean, inv_std = (float)(1 / sqrt(M2 / count + eps)).
 * AUV_EINVAL: device < 0; obs_dim outside [1, 16384]; n_slots < 1; a NULL pointer; mom not 8-byte, table not 8-byte aligned; eps < 0
 * or not finite.  The caller orders the launch behind every chain's last launch and in front of the next rollout's first (as auv_gae).
 *
 * auv_norm_returns is the reward pass over a stored rollout R[T][N] / Dn[T][N] (row-major, as auv_gae), at most three launches on
 * `stream`, ordered by the caller like the fold:
 *   update != 0   (1) one thread per environment walks t = 0 .. T - 1:  ret = ret * gamma + R[t] in fp64, the return taken into a
 *                 Welford recursion over its T returns (d = ret - mean; mean += d / (t + 1); M2 += d * (ret - mean)), THEN ret = 0
 *                 where Dn[t] != 0 (stable-baselines' order); ret[N] f64 is carried to the next call, rpart[N][2] f64 = (mean, M2)
 *                 is scratch.  (2) one wave merges the N partials, each of count T, into rmom[3] f64 = (count, mean, M2): lane l the
 *                 environments l, l + 64, ... in that order, then the tree and the merge into the running moments as above.
 *   always        (3) R_out[i] = min(max(R[i] / (float)sqrt(M2 / count + eps), -clip_reward), clip_reward), an f32 division, with
 *                 the UPDATED moments; R_out may be R.  update == 0 (VecNormalize.training == False) runs (3) alone: ret, rpart and
 *                 rmom are not written (ret and rpart may then be NULL).
 * AUV_EINVAL: device < 0; T < 1 or N < 1; R, R_out or rmom NULL; update with Dn, ret or rpart NULL; a float buffer not 4-byte or a
 * double buffer not 8-byte aligned; clip_reward not > 0; gamma or eps not finite, eps < 0.                                          */
typedef struct auv_policy_norm {
  auv_policy_io_t io;
  const float* table;        /* [obs_dim][2]: mean, inv_std                                                    */
  float* part;               /* [T * part_ld][2][obs_dim]                                                      */
  int32_t* pcnt;             /* [T * part_ld]                                                                  */
  int32_t part_ld, part_base;
  float clip_obs;
  int32_t reserved;
} auv_policy_norm_t;
int auv_policy_act_norm(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_norm_t* io, void* stream);
int auv_policy_act_norm_arch(auv_handle_t* h, int32_t e0, int32_t ne, const auv_policy_norm_t* io, const auv_policy_arch_t* arch, void* stream);
int auv_policy_rollout_norm(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams, const auv_policy_norm_t* ios,
                            float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0,
                            const int64_t* gstep0);
int auv_policy_rollout_norm_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                                 const auv_policy_norm_t* ios, const auv_policy_arch_t* arch, float* obs_dev, float* reward_dev,
                                 uint8_t* done_dev, int32_t n_steps, int32_t flush, const int64_t* t0, const int64_t* gstep0);
int auv_norm_rows(int32_t device, const float* X, const int64_t* idx, int64_t ldx, const float* table, float clip_obs, float* out,
                  int64_t ldo, int32_t M, int32_t obs_dim, void* stream);
int auv_norm_fold(int32_t device, const float* part, const int32_t* pcnt, int32_t n_slots, int32_t obs_dim, double eps, double* mom,
                  float* table, void* stream);
int auv_norm_returns(int32_t device, const float* R, const float* Dn, float* R_out, int32_t T, int32_t N, double gamma, float clip_reward,
                     double eps, double* ret, double* rpart, double* rmom, int32_t update, void* stream);

/* ---- a population of policies: one weight block per group of rows (csrc/k11_population.hip) ---------------------------------------
 * A MEMBER is the packed policy net of auv_policy_io::params -- W1 b1 W2 b2 W3 b3 W4 b4 in MFMA fragment order, what the first
 * net of that buffer holds -- auv_population_member_floats(obs_dim) floats (the net rounded up to a multiple of 4 floats).  Members
 * lie `stride` floats apart.  Row j of a launch belongs to member j / G and is evaluated with the block members + (j / G) * stride; G
 * (rows per member) is a multiple of 16, so a 16-row tile -- one workgroup -- never straddles two members.  The matrix chains are
 * those of auv_policy_eval: for the same row and the same block the mean has the same bits.  Deterministic: no value net, no
 * sampling, no rollout stores.
 *   outputs     each nullable, written for rows < M only:  mu[j][2];  action[j * action_ld + c] = act_mid[c] + act_half[c] *
 *               clip(mu[c], clip_lo[c], clip_hi[c]) (auv_policy_eval's expression).
 *   accumulate  != 0: before the matrix work the launch reads reward_in[j] and done_in[j] -- the step row j's environment has just
 *               completed -- and at its end stores fit[j] = fit[j] + reward_in[j] (one rounded float32 add per launch) and ends[j] =
 *               ends[j] + (done_in[j] != 0).  Needs all four buffers.
 *   act         != 0: the nets are evaluated and the outputs written; 0: the launch only accumulates (the flush behind a
 *               window's last step) and X, mu and action are not touched.
 * AUV_EINVAL, before anything is enqueued: G not a positive multiple of 16; members NULL or not 16-byte aligned; stride smaller than
 * auv_population_member_floats(obs_dim) or not a multiple of 4; obs_dim < 1 or too wide for the kernel's LDS tile (auv_policy_eval's
 * rule); with act: X NULL, ldx < obs_dim, action with action_ld < 2, neither output and no accumulation; without act: no
 * accumulation; accumulate with one of its buffers NULL; M < 0; a buffer that is not 4-byte aligned.  M == 0 succeeds and launches
 * nothing.  Enqueued on `stream`; no synchronisation, no allocation.  All pointers except `io` are device pointers.                  */
typedef struct auv_population_io {
  const float* members;      /* [P][stride], P >= ceil(M / G) members                                            */
  const float* X;            /* observation rows, row stride ldx floats                                          */
  float* mu;                 /* [M][2]         (nullable)                                                        */
  float* action;             /* [M][action_ld] (nullable)                                                        */
  const float* reward_in;    /* [M]  accumulation: the environment's reward buffer                               */
  const uint8_t* done_in;    /* [M]  accumulation: the environment's done buffer                                 */
  float* fit;                /* [M]  accumulation: running sum of rewards                                        */
  int32_t* ends;             /* [M]  accumulation: running count of dones                                        */
  int64_t stride, ldx;       /* floats                                                                           */
  int32_t G, M, obs_dim, action_ld;
  int32_t accumulate, act;
  float act_mid[2], act_half[2], clip_lo[2], clip_hi[2];   /* action = mid + half * clip(mu, lo, hi)          */
} auv_population_io_t;
size_t auv_population_member_floats(int32_t obs_dim);
int auv_population_act(int32_t device, const auv_population_io_t* io, void* stream);
/* n_steps steps of every slice with ONE call: per step and slice the population launch and the environment's step of that slice, back
 * to back on streams[i] (auv_policy_rollout's loop).  ios[i] is written in WHOLE-BATCH rows -- row j is environment j, M = N, action
 * the environment's [N][action_ld] float32 action buffer (8-byte aligned), fit / ends [N] -- and the call itself takes the slice's
 * rows of it; X, ldx, reward_in, done_in, accumulate and act of ios[i] are not read: rows come from obs_dev, rewards and dones from
 * reward_dev / done_dev.  The first launch of a call does not accumulate, every later one adds the step before it; `flush` != 0: a
 * final accumulate-only launch per slice adds the last step.  Slice bounds must be multiples of ios[i].G (AUV_EINVAL).  The chains are
 * not ordered against each other or the caller's stream.                                                                         */
int auv_population_rollout(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                           const auv_population_io_t* ios, float* obs_dev, float* reward_dev, uint8_t* done_dev, int32_t n_steps,
                           int32_t flush);
/* Members from a base block, on the device (mirrored sampling): member p of generation g is
 *   members[p * stride + i] = theta[i] + s_p * (sigma * eps(seed, g, p / 2, i)),   s_p = +1 for even p, -1 for odd p,
 * two rounded float32 operations in that association.  eps is counter-based and free of transcendental functions, so that a host
 * mirror reproduces it bit for bit (gym_auv_amd/population.py: es_noise):
 *   h = mix(mix(mix(seed ^ g * 0xd1342543de82ef95) ^ pair) ^ i)   (mix: the splitmix64 finaliser, 64-bit wrap-around arithmetic)
 *   S = the sum of the four 16-bit fields of h;   eps = float32(S - 131070) * c,   c = float32(1 / sqrt(4 (65536^2 - 1) / 12))
 * -- symmetric, unit variance, |eps| <= 131070 c ~ 3.464.  PADDING elements of the block -- the columns of W1 beyond obs_dim, rows
 * 2..15 of W4, entries 2..15 of b4 -- get no noise: they keep theta's value (zero); the tail [member_floats, stride) is set to zero.
 * theta: auv_population_member_floats(obs_dim) floats; theta and members 16-byte aligned, stride a multiple of 4 and >= the block;
 * P >= 1 (an odd P leaves the last pair half used); sigma finite.                                                                  */
int auv_population_perturb(int32_t device, const float* theta, float* members, int64_t stride, int32_t P, int32_t obs_dim, float sigma,
                           uint64_t seed, int64_t generation, void* stream);
/* The ES gradient estimate with eps regenerated from the counters (nothing of the noise is stored):
 *   grad[i] = (1 / (P sigma)) * sum over pair = 0 .. P / 2 - 1 of (w[2 pair] - w[2 pair + 1]) * eps(seed, g, pair, i)
 * one float32 accumulator per element, pairs in increasing order, per pair one rounded difference, one rounded product and one rounded
 * add; the factor last, as acc * float32(1 / (P sigma)) (the quotient formed in double).  Padding elements get exactly 0.  lr != 0:
 * also theta[i] = theta[i] + lr * grad[i] (ascent; two rounded operations; padding untouched).  w: [P] float32 device, the shaped
 * fitness; P even and >= 2; sigma finite and > 0; theta (needed with lr != 0) and grad: one member block each, 16-byte aligned.     */
int auv_population_update(int32_t device, float* theta, const float* w, float* grad, int32_t P, int32_t obs_dim, float sigma, float lr,
                          uint64_t seed, int64_t generation, void* stream);
/* The population at the other hidden widths of the forward launches (auv_policy_arch_t above; kernels: csrc/k14_population_arch.hip,
 * the same bodies as k11's, csrc/auv_population_pass.h).  A member is then the packed policy net obs -> h1 -> h2 -> h3 -> 2 of
 * auv_policy_param_floats_arch's layout: auv_population_member_floats_arch(obs_dim, arch) floats,
 *   h1 * K0p + h1 + h2 * h1 + h2 + h3 * h2 + h3 + 16 * h3 + 16 rounded up to a multiple of 4,   K0p = obs_dim rounded up to 32,
 * and the padding elements that get no noise and no gradient are those of that layout.  Every word, every check in its order and
 * every error of the entries above holds, with the member size and the LDS tile of the triple; for the same row and the same block the
 * mean has the bits of auv_policy_eval_arch at that triple; the noise does not depend on the widths.  AUV_EINVAL before anything is
 * enqueued: arch NULL, or a triple outside the list -- it is never rounded to a listed one, and auv_population_member_floats_arch
 * then returns 0 (as it does for obs_dim <= 0).  (256, 128, 64) through an _arch entry runs the very kernels of the entry without
 * the suffix.                                                                                                                    */
size_t auv_population_member_floats_arch(int32_t obs_dim, const auv_policy_arch_t* arch);
int auv_population_act_arch(int32_t device, const auv_population_io_t* io, const auv_policy_arch_t* arch, void* stream);
int auv_population_rollout_arch(auv_handle_t* h, int32_t n_slices, const int32_t* bounds, void* const* streams,
                                const auv_population_io_t* ios, const auv_policy_arch_t* arch, float* obs_dev, float* reward_dev,
                                uint8_t* done_dev, int32_t n_steps, int32_t flush);
int auv_population_perturb_arch(int32_t device, const float* theta, float* members, int64_t stride, int32_t P, int32_t obs_dim, float sigma,
                                uint64_t seed, int64_t generation, const auv_policy_arch_t* arch, void* stream);
int auv_population_update_arch(int32_t device, float* theta, const float* w, float* grad, int32_t P, int32_t obs_dim, float sigma, float lr,
                               uint64_t seed, int64_t generation, const auv_policy_arch_t* arch, void* stream);

/* Generalised advantage estimation over a rollout of T steps x N environments (row-major [T][N] device buffers; V and
 * last_v in the same units as R): adv and ret = adv + V, one launch on `stream`.                                       */
int auv_gae(auv_handle_t* h, const float* R, const float* V, const float* Dn, const float* last_v, float gamma, float lam,
            float* adv_out, float* ret_out, int32_t T, int32_t N, void* stream);

/* ---- snapshot / restore: copy environments out of a handle and back in, on the device ------------------------------------
 * (The reference has no such call: its environment is a Python object, copied with copy.deepcopy.  Here an environment is rows of a
 * dozen device buffers plus a binding to a world of the bank.)  A SNAPSHOT ROW is everything that makes environment e what it is
 * between two calls, packed into auv_snapshot_row_bytes(h) bytes of caller-owned device memory.  Opaque to the caller; the layout,
 * for the record (offsets in bytes; every part starts on a multiple of 16 and is padded with zero bytes to the next one):
 *      0  counters      int32[4]   t_step, vessel step counter, episodes, pad            (AUV_FIELD_COUNTERS)
 *     16  state         f64[6]     x, y, psi, u, v, r -- the environment's column of the [6][N] array
 *     64  reward64, path-following term, LiDAR term of the reward   f64[3]
 *     88  world index   int32;  92  collision  uint8;  93..95 zero
 *     96  info64 f64[8] | nav64 f64[8] | step_info f64[4] | episode f64[4]
 *    288  lidar_d f64[S] | obs64 f64[6 + S] | mover f64[Mmax][4] | cull limits int32[Kmax][2] | nearby uint8[Kmax] |
 *         sector_d f64[n_sectors] (pooled observations only)
 * i.e. every per-environment buffer a later step, or a later auv_read of any field, can observe.  NOT in a row: the hand-over records
 * of the one-launch and multi-step shapes (their marks are down between launches), AUV_FIELD_BROKEN, the episode log, the position in
 * the action ring, the diagnostic stamps, and anything per WORLD -- a row names its world by index only.
 *   auv_snapshot   row j of rows_dev <- environment env_idx_dev[j]  (env_idx_dev == NULL: environment j, m <= N).  rows_dev: m rows,
 *                  16-byte aligned.
 *   auv_restore    environment env_idx_dev[j] <- row row_idx_dev[j] of the n_rows rows at rows_dev (either NULL: j), for j < m.  One row
 *                  may feed many environments (a FORK); an environment named twice gets one of its rows, which one is not defined.  The
 *                  environment's world descriptor is rebuilt from the row's world index and THIS handle's bank, so a row is valid in any
 *                  handle with the same layout.  obs_dev (nullable): the caller's [N][obs_dim] float32 observation buffer; the rows of
 *                  the restored environments are written exactly as the step that produced the snapshot state wrote them.
 *   auv_snapshot_layout   fingerprint of the layout: a hash of AUV_ABI_VERSION, the snapshot format number, n_sensors, Kmax, Mmax,
 *                  n_sectors, obs_channels, use_lidar, the number of worlds and the row size (0 before a bank is loaded).  auv_restore
 *                  returns AUV_EINVAL for a `layout` that is not the handle's own: that check is what makes a restore memory-safe.
 *                  Whether two banks with the same fingerprint hold the same WORLDS is the caller's promise.
 * One launch each, stream-ordered, no allocation, no host synchronisation; one wave per row (csrc/k7_snapshot.hip).  A pair whose
 * environment, row or world index is out of range is skipped -- never accessed -- and counted: auv_snapshot_skipped reads the count
 * (since the bank was loaded; synchronises `stream`).  Refused before anything is enqueued: no bank (AUV_ESTATE); a fresh world per
 * reset (AUV_ESTATE: a bank slot belongs to one environment there); a pending auv_step_async (AUV_ESTATE); a pending hand-over
 * time-out is recovered from first and reported as by the step calls.  Ordering against step launches on OTHER streams is the
 * caller's, as for auv_read / auv_write.  Eager only.                                                                        */
size_t auv_snapshot_row_bytes(const auv_handle_t* h);
uint64_t auv_snapshot_layout(const auv_handle_t* h);
int auv_snapshot(auv_handle_t* h, const int32_t* env_idx_dev, int32_t m, void* rows_dev, void* stream);
int auv_restore(auv_handle_t* h, uint64_t layout, const void* rows_dev, int32_t n_rows, const int32_t* row_idx_dev,
                const int32_t* env_idx_dev, int32_t m, float* obs_dev, void* stream);
int auv_snapshot_skipped(auv_handle_t* h, int64_t* out_skipped, void* stream);

/* Scores of the candidate action sequences of a shooting planner (gym_auv_amd/planning.py), from the [n_steps][n] record of an
 * auv_step_multi_record launch: score[e] = sum over t of disc_t * reward_rec[t][e], up to AND INCLUDING the first t with
 * done_rec[t][e]; disc_0 = 1, disc_{t+1} = disc_t * gamma.  Every product and every sum is rounded to float32, in increasing t,
 * without contraction: part of the contract, a plain float32 loop gives the same bits.  best[g], g < n / group: the index WITHIN
 * group g (environments g * group .. (g + 1) * group - 1) of its largest score; the lowest index wins a tie, a NaN score never
 * wins (all NaN: 0).  One launch on `stream`; n a multiple of group.                                                         */
int auv_plan_score(auv_handle_t* h, const float* reward_rec, const uint8_t* done_rec, int32_t n_steps, int32_t n, int32_t group,
                   float gamma, float* score_dev, int32_t* best_dev, void* stream);
/* The same with a terminal value (MPC with a learned critic): auv_plan_score's contract, word for word, and in addition an
 * environment with NO done in [0, n_steps) adds float32(disc_T * terminal_value[e]), disc_T being the same running product after
 * n_steps multiplications -- one more rounded product and one more rounded sum, last in order.  A candidate that saw a done never
 * reads its terminal value (a NaN there cannot reach its score).  terminal_value [n] float32 on the device; NULL: auv_plan_score. */
int auv_plan_score_v(auv_handle_t* h, const float* reward_rec, const uint8_t* done_rec, int32_t n_steps, int32_t n, int32_t group,
                     float gamma, const float* terminal_value, float* score_dev, int32_t* best_dev, void* stream);

/* The planner's sampler and refit on the device (csrc/k15_plan.hip; gym_auv_amd/planning.py: reference_plan_sample and
 * reference_plan_refit are the same arithmetic in NumPy).  n = B * group planner environments, environment e = b * group + k being
 * candidate k of group b; mean / sigma / chosen are [n_steps][B][2] float32, the ring [n_steps][n][2] float32.  All arithmetic is
 * float32, round to nearest, without contraction, in the order stated: the orders are part of the contract.  One launch each on
 * `stream`, no allocation, no host synchronisation.  1 <= group <= AUV_PLAN_MAX_GROUP, n a multiple of group, n_steps * n * 2 < 2^31,
 * every pointer 4-byte aligned; a failed check returns AUV_EINVAL and launches nothing.
 *   auv_plan_sample   ring[t][e][j] = clip(m + s * eps), one rounded product, one rounded sum, then fmaxf(fminf(., hi[j]), lo[j]);
 *                     candidate k = 0 is clip(m), without noise.  m, s = mean, sigma at row min(t + shift, n_steps - 1) of group b:
 *                     shift 0, or 1 for a receding-horizon warm start (the previous plan moved on one step, its last step repeated).
 *                     eps = the noise of auv_population_perturb at (seed, generation = draw, pair = e, element = 2 t + j).  reset_dev
 *                     (nullable, [B] bytes): a group with reset[b] != 0 reads row t -- no shift -- of mean0 / sigma0 instead (both
 *                     required with a mask, ignored without).  lo_host, hi_host: two floats each, on the host.
 *   auv_plan_refit    chosen[t][b][:] = ring[t][b * group + best[b]][:] and predicted[b] = score[b * group + best[b]] (each nullable;
 *                     best[b] is clamped into the group), and, with mean_out / sigma_out (both or neither; buffers of their own,
 *                     not the inputs), the next sampling distribution of every group:
 *                     AUV_PLAN_CEM   the elite are the n_elite first candidates in the total order of the scorer's argmax: larger score
 *                       first, lower index on a tie; a NaN score ranks below every number, NaNs among themselves by index.  Per (t, j),
 *                       over the elite in ascending candidate index: s = the sequential sum of a, mean = s / n_elite; q = the
 *                       sequential sum of (a - mean) * (a - mean), difference, product and sum each rounded;
 *                       sigma = fmaxf(sqrt(q / n_elite), sigma_min).  1 <= n_elite <= group.  mean_in / sigma_in are not read.
 *                     AUV_PLAN_MPPI  w_k = 1 where score_k equals the group's largest valid score, else expf((score_k - max) / lambda)
 *                       (difference and quotient rounded), 0 for a NaN score; mean = (sum_k w_k * a_k) / (sum_k w_k), both sums
 *                       sequential over ALL candidates in ascending k, every product rounded; sigma_out = sigma_in.  A group without
 *                       a valid score keeps mean_in.  lambda finite and > 0.  expf is the device's: reproducible run to run, not
 *                       bit for bit on a host -- except where every weight but the maxima's underflows to 0.                       */
#define AUV_PLAN_CEM 0
#define AUV_PLAN_MPPI 1
#define AUV_PLAN_MAX_GROUP 1024
int auv_plan_sample(auv_handle_t* h, const float* mean_dev, const float* sigma_dev, const float* mean0_dev, const float* sigma0_dev,
                    const uint8_t* reset_dev, int32_t n_steps, int32_t n, int32_t group, int32_t shift, const float* lo_host,
                    const float* hi_host, uint64_t seed, uint64_t draw, float* ring_dev, void* stream);
int auv_plan_refit(auv_handle_t* h, const float* ring_dev, const float* score_dev, const int32_t* best_dev, int32_t n_steps, int32_t n,
                   int32_t group, int32_t method, int32_t n_elite, float sigma_min, float lambda, const float* mean_in_dev,
                   const float* sigma_in_dev, float* mean_out_dev, float* sigma_out_dev, float* chosen_dev, float* predicted_dev,
                   void* stream);

/* ---- the PPO update (scripts/run.py:332-357: PPO2 with MlpPolicy, net_arch [256, 128, 64] for policy and value
 * function, tanh, a diagonal Gaussian with a free log_std[2]): one minibatch step of examples/ppo.py (minibatch_step) as a few
 * launches -- forward and backward of both nets on the matrix cores in exact f32, the clipped-surrogate / value / entropy loss, the
 * two global-norm clips and Adam (csrc/k8_ppo_update.hip).  The updater is an object of its own: it needs no environment handle.
 *   auv_ppo_param_floats   length of the flat parameter / gradient / moment vectors, in TORCH layout: the policy net's W1 [256][D] b1
 *                    [256] W2 [128][256] b2 W3 [64][128] b3 W4 [2][64] b4 [2], the value net's W1 .. W4 [1][64] b4 [1], log_std[2].
 *   auv_ppo_create   allocates the packed weight copies and the scratch of batches up to max_batch rows (about 8.5 KB per row at
 *                    obs_dim 186).  AUV_EINVAL for obs_dim < 1 or an observation too wide for the row pass' LDS tile.
 *   auv_ppo_load     packs the forward (the layout of auv_policy_io::params) and the transposed fragment-order copy from theta, and the
 *                    attached policy buffer: after initialisation, and after any change of theta made elsewhere.
 *   auv_ppo_attach_policy   policy_params: a buffer of auv_policy_param_floats(obs_dim) floats, 16-byte aligned, whose padding is zero
 *                    (NULL: detach).  auv_ppo_load and every auv_ppo_adam then write each weight into it as well: what
 *                    FusedActorCritic.refresh() does with a permuted copy per layer.
 *   auv_ppo_grad     grad (flat layout) <- d loss / d theta over the B rows idx[0 .. B) of the n_rows stored transitions.  An index
 *                    outside [0, n_rows) is the caller's error: it is not checked.  stats[8]: loss, pg, vf, max |adv|, max ratio, the
 *                    number of non-finite inputs among the gathered rows, the fraction of rows on the clipped branch, 0.
 *   auv_ppo_adam     coef = min(1, max_norm / (norm + 1e-6)) per group (policy net + log_std | value net; norms_out[2]: the norms before
 *                    clipping), then Adam as torch.optim.Adam formulates it (amsgrad off, no weight decay) on theta, m, v, and the
 *                    scatter of every updated weight into the packed copies and the attached buffer.  `grad` is not modified.
 * grad and adam are separate so that data-parallel training can all-reduce the flat gradient in between.  Deterministic: no
 * floating-point atomics, every reduction in an order fixed by B; two calls on the same inputs give the same bits.  Everything is
 * enqueued on `stream`, nothing synchronises; all pointers except the two structs are device pointers.                      */
typedef struct auv_ppo auv_ppo_t;
typedef struct auv_ppo_batch {
  const float* O;            /* [n_rows][obs_dim]                                                            */
  const float* A;            /* [n_rows][2]                                                                  */
  const float* LP;           /* [n_rows]  log-probability under the policy that collected the rows           */
  const float* ADV;          /* [n_rows]  (normalised) advantages                                            */
  const float* RET;          /* [n_rows]  value targets                                                      */
  const int64_t* idx;        /* [B] rows of the minibatch; NULL: rows 0 .. B - 1                             */
  int32_t B, n_rows;
  float clip, vf_coef, ent_coef;
} auv_ppo_batch_t;
typedef struct auv_ppo_adam {
  double lr, beta1, beta2, eps;      /* double: 1 - beta2 is rounded to float once, from here, as torch rounds it */
  double bc1, bc2;                   /* 1 - beta1^t, 1 - beta2^t of this step t >= 1, computed on the host; double for the same
                                        reason: lr / bc1 and sqrt(bc2) reach the kernel as the floats torch.optim.Adam uses      */
  float max_norm_pi, max_norm_v;     /* <= 0: no clipping                                                     */
} auv_ppo_adam_t;
size_t auv_ppo_param_floats(int32_t obs_dim);
int auv_ppo_create(int32_t device, int32_t obs_dim, int32_t max_batch, auv_ppo_t** out);
void auv_ppo_destroy(auv_ppo_t* p);
int auv_ppo_load(auv_ppo_t* p, const float* theta, void* stream);
int auv_ppo_attach_policy(auv_ppo_t* p, float* policy_params);
int auv_ppo_grad(auv_ppo_t* p, const auv_ppo_batch_t* batch, float* grad, float* stats, void* stream);
int auv_ppo_adam(auv_ppo_t* p, float* theta, float* m, float* v, const float* grad, const auv_ppo_adam_t* adam, float* norms_out,
                 void* stream);
/* The update at the other hidden widths of the forward launches (auv_policy_arch_t above; scripts/run.py:332-357 trains
 * net_arch [256, 128, 64] only): the updater remembers its triple, and auv_ppo_load / attach_policy / grad / grad_clone / adam then act
 * on obs -> h1 -> h2 -> h3 -> out with (h1, h2, h3) in the place of (256, 128, 64) in every layout above (kernels:
 * csrc/k13_ppo_update_arch.hip; (256, 128, 64) runs the very kernels of auv_ppo_create's updaters).  The attached buffer holds
 * auv_policy_param_floats_arch(obs_dim, arch) floats: its length is the caller's to match, it cannot be checked here.
 *   auv_ppo_param_floats_arch   auv_ppo_param_floats for the triple; 0 for obs_dim <= 0, arch NULL or a triple outside the list.
 *   auv_ppo_create_arch         auv_ppo_create for the triple; AUV_EINVAL, before any device call, also for arch NULL or a triple
 *                               outside the list (never rounded to a listed one).                                                */
size_t auv_ppo_param_floats_arch(int32_t obs_dim, const auv_policy_arch_t* arch);
int auv_ppo_create_arch(int32_t device, int32_t obs_dim, int32_t max_batch, const auv_policy_arch_t* arch, auv_ppo_t** out);

/* ---- the supervised (clone) row pass of the same updater: the policy trained towards given target actions, the value net towards
 * given targets -- distilling a planner's decisions (gym_auv_amd/planning.py, DistillBuffer), cloning an autopilot, warm-starting PPO.
 *   auv_ppo_grad_clone   auv_ppo_grad's contract (flat torch-layout gradient over the B rows idx[0 .. B) of n_rows stored rows,
 *                    indices unchecked, everything enqueued on `stream`, deterministic) with another head.  With w_i the row's weight
 *                    (1 without W), sigma_k = exp(log_std_k), z_ik = (a_ik - mu_ik) / sigma_k:
 *                      kind 0   bc = (1/B) sum_i w_i sum_k (0.5 z_ik^2 + log_std_k + log sqrt(2 pi))      the Gaussian NLL of A
 *                      kind 1   bc = (1/B) sum_i w_i sum_k 0.5 (a_ik - mu_ik)^2                            log_std gets no bc gradient
 *                      vf = (1/B) sum_i w_i 0.5 (v_i - ret_i)^2;  loss = bc + vf_coef vf - ent_coef sum_k (0.5 + log sqrt(2 pi) + log_std_k)
 *                    A is in the policy's own space: the mean BEFORE the affine action map and its clip.  A row of weight 0 adds
 *                    exactly nothing.  stats[8]: loss, bc, vf, max |a - mu| over the rows of weight > 0, the sum of the weights, the
 *                    number of non-finite values among the gathered rows of O, A, RET and W, 0, 0.
 *                    AUV_EINVAL: B < 1, B > max_batch, a kind other than 0 / 1, a null O, A or RET.
 * auv_ppo_adam applies the gradient as it applies auv_ppo_grad's: the packed copies and the attached policy buffer follow every
 * clone step too, and clone and PPO steps may alternate on one updater.                                                          */
typedef struct auv_ppo_clone_batch {
  const float* O;            /* [n_rows][obs_dim]                                                            */
  const float* A;            /* [n_rows][2]  target actions, in the policy's own (pre-action-map) space      */
  const float* RET;          /* [n_rows]     value targets                                                   */
  const float* W;            /* [n_rows]     row weights >= 0; NULL: all one                                 */
  const int64_t* idx;        /* [B]; NULL: rows 0 .. B - 1                                                   */
  int32_t B, n_rows, kind;   /* kind 0: Gaussian NLL, 1: MSE on the mean                                     */
  float vf_coef, ent_coef;
} auv_ppo_clone_batch_t;
int auv_ppo_grad_clone(auv_ppo_t* p, const auv_ppo_clone_batch_t* batch, float* grad, float* stats, void* stream);

/* ---- the PPO row pass for a tanh-squashed policy (auv_policy_*_squash above): auv_ppo_grad's contract, batch layout and gradients with
 * the entropy of the SQUASHED distribution in the place of the Gaussian's, estimated on the stored rows:
 *     loss  = pg + vf_coef vf - ent_coef (1/B) sum_i ent_i
 *     ent_i = sum_k [0.5 + log sqrt(2 pi) + log_std_k + log(1 - tanh^2(u_ik))],   u_ik = mu_ik + sigma_k sg(z_ik),  z = (a - mu) / sigma
 * sg: stop-gradient, so u_ik has the VALUE of the stored action a_ik and the gradient of a reparameterised sample; log(1 - tanh^2 u)
 * is evaluated as 2 (log 2 - |u| - log1p(exp(-2 |u|))), finite for every finite u.  On top of auv_ppo_grad's gradients:
 *     d loss / d mu_ik     += ent_coef 2 tanh(a_ik) / B
 *     d loss / d log_std_k  = (PPO's) - ent_coef (1 - (1/B) sum_i 2 tanh(a_ik) (a_ik - mu_ik))       in the place of (PPO's) - ent_coef
 * A holds PRE-SQUASH actions and LP their Gaussian log-density, as the squash launches store them: pg needs no Jacobian.  stats[8] as
 * auv_ppo_grad's with slot 7 = (1/B) sum_i ent_i.  With ent_coef == 0 the gradient has the bits of auv_ppo_grad's on the same batch.
 * A non-finite a counts as a bad input, as there.  The type selects the head; the fields are auv_ppo_batch_t's.                   */
typedef struct auv_ppo_squash_batch {
  const float* O;            /* [n_rows][obs_dim]                                                            */
  const float* A;            /* [n_rows][2]  stored (pre-squash) actions u                                   */
  const float* LP;           /* [n_rows]     Gaussian log-density of u under the collecting policy           */
  const float* ADV;          /* [n_rows]                                                                     */
  const float* RET;          /* [n_rows]                                                                     */
  const int64_t* idx;        /* [B]; NULL: rows 0 .. B - 1                                                   */
  int32_t B, n_rows;
  float clip, vf_coef, ent_coef;
} auv_ppo_squash_batch_t;
int auv_ppo_grad_squash(auv_ppo_t* p, const auv_ppo_squash_batch_t* batch, float* grad, float* stats, void* stream);

/* ---- rendering: rgb_array frames of B environments, drawn on the device (BaseEnvironment.render, environment.py:410-437; the
 * reference draws ONE environment on the host with pygame: a vessel-centred top view, render2d/renderer.py:62-120) -------------
 * frames_dev [B][H][W][3] uint8 <- a top view of environment env_idx_host[j] (any environments, repeats allowed), centred on
 * the vessel, `zoom` pixels per metre, screen y downwards.  view: AUV_VIEW_HEADING_UP (the heading points up) or
 * AUV_VIEW_NORTH_UP (world x to the right, world y up).  Two launches on `stream` (csrc/k10_render.hip): a geometry pass, one
 * wave per frame, and the rasteriser, one workgroup per 16 x 16 tile.  The index list is copied into a pinned buffer of the
 * handle before the call returns (the caller's list may go at once) and travels from there by an asynchronous copy.  The geometry
 * lives in scratch of the handle (some 40 S + 160 Mmax bytes per frame), shared by all calls: renders of one handle must be
 * ordered against each other -- one stream, or events between streams.  HOST SYNCHRONISATION: none in the steady state.  The first
 * call, a call with more frames than any call before it, and loading a new bank drain the device and (re)allocate that scratch;
 * and a call waits for the render four calls back if that one has not started yet.  Eager only (not inside a stream capture).
 * THE PIXEL RULE -- the contract; gym_auv_amd/render.py (render_reference) restates it in NumPy bit for bit.  IEEE fp64, no
 * contraction, no square root.  The centre of pixel (row i, column j) is the world point
 *     p = (x, y) + M (j + 0.5 - W / 2, i + 0.5 - H / 2),   cam = x, y, M00, M01, M10, M11, zoom, view
 * M in metres per pixel: heading up (s / zoom, -c / zoom; -c / zoom, -s / zoom) with (s, c) the device's sincos of psi, north up
 * (1 / zoom, 0; 0, -1 / zoom).  Layers, later ones overwrite: background, path, trail, static obstacles, markers, movers,
 * LiDAR beams, vessel.
 *     line    (path, trail, beams)  e = b - a, t = clamp(((p - a) . e) / (e . e), 0, 1) with one division (t = 0 when e . e is
 *             not > 0), lit when |(p - a) - t e|^2 <= h^2, h = 0.5 line_px / zoom
 *     filled  (obstacles, movers, vessel; per shape)  lit when an odd number of its boundary segments (ax, ay, bx, by) have
 *             (ay > py) != (by > py) and px < ax + (py - ay) * (bx - ax) / (by - ay).  Circles are their stored 64-gons.
 *     disc    (markers: x, y, radius)  (px - x)^2 + (py - y)^2 <= radius^2
 * Among several lit beams the highest index wins; a beam's channel is (lo * (255 - q) + hi * q + 127) / 255 in integers between
 * palette rows 6 and 7, q = min(255, int(max(0, closeness) * 255 + 0.5)) (the beam's closeness column of the observation row; the
 * linear rule 1 - clip(range / sensor_range, 0, 1) with pooled observations, which keep no such column).  With the LiDAR off nothing
 * was measured: every beam has length 0 and lies under the vessel.
 *   trail_dev    [B][L][2] fp64 or NULL: positions joined by line segments; the first row with a NaN ends a frame's trail.
 *   markers_dev  [B][M][3] fp64 or NULL: x, y, radius.
 *   palette_host [9][3] uint8: background, path, trail, obstacle, marker, mover, beam lo, beam hi, vessel.
 *   cam_out [B][8], dyn_seg_out [B][5 Mmax + 5][4] (every mover's pentagon -- zeros for the slots past the world's movers -- then
 *   the vessel's), ray_seg_out [B][S][4] (vessel -> end of beam), ray_q_out [B][S] uint8: fp64 device buffers or NULL; what the
 *   geometry pass made of the state, i.e. everything the rasteriser reads besides the bank's tables.
 * AUV_EINVAL: B, H or W < 1, H or W > 4096, B > 65535, an index outside [0, N), a zoom or line width that is not finite and > 0,
 * an unknown view, a NULL palette or frame buffer, L or M < 0, a handle with no bank loaded.                                 */
enum { AUV_VIEW_HEADING_UP = 0, AUV_VIEW_NORTH_UP = 1 };
int auv_render(auv_handle_t* h, void* stream, const int32_t* env_idx_host, int32_t B, int32_t H, int32_t W, double zoom, int32_t view,
               double line_px, const double* trail_dev, int32_t L, const double* markers_dev, int32_t M, const uint8_t* palette_host,
               uint8_t* frames_dev, double* cam_out, double* dyn_seg_out, double* ray_seg_out, uint8_t* ray_q_out);

int32_t auv_abi_version(void);
const char* auv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* AUV_HIP_H */
