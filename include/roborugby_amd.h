/*
 * roborugby_amd.h -- C-ABI of the MI355X-native batched RoboRugby simulator.
 *
 * The reference (harman097/RoboRugby) has no FFI: its boundary is the gym.Env Python API
 * (`reset/step/get_game_state`, robo_rugby/gym_env/RR_EnvBase.py:202-216,260-297,550-559).  This
 * header is the thin C layer beneath the Python mirror of that API (roborugby_amd/env.py): plain
 * pointers and sizes, no torch types.  Every data pointer is a DEVICE pointer owned by the caller
 * (PyTorch-ROCm allocations); every call is enqueued on `stream` (a hipStream_t, NULL = default
 * stream) and returns without synchronising.  One handle per (process, device); a handle is not
 * re-entrant.  Return value: 0 = OK, <0 = API misuse (see rr_last_error()).  Physics faults -- the
 * places where the reference raises from inside step() -- never cross the ABI as errors: they are
 * reported per arena in `status` (RR_STATUS_* bits).
 *
 * Shapes use N = num_envs, NR = nr_happy + nr_grumpy, NB = nb_pos + nb_neg.
 */
#ifndef ROBORUGBY_AMD_H
#define ROBORUGBY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 4

/* per-arena status bits; each mirrors one exception site of the reference */
#define RR_STATUS_BOT_RESOLVE_FAIL 1   /* RR_EnvBase.py:313  "UNABLE TO RESOLVE BOT/BOT COLLISIONS"   */
#define RR_STATUS_BOT_STUCK 2          /* RR_EnvBase.py:328  "ROBOTS STUCK FROM PRIOR FRAME"          */
#define RR_STATUS_UNDO_MOVE_FAIL 4     /* RR_EnvBase.py:325  "UNABLE TO UNDO MOVE FOR ROBOT"          */
#define RR_STATUS_UNDO_FAIL 8          /* RR_EnvBase.py:421  "UNABLE TO RESOLVE ALL COLLISIONS..."    */
#define RR_STATUS_SAME_SPOT 16         /* RR_TrashyPhysics.py:250 balls in the exact same spot        */
#define RR_STATUS_DIV0 32              /* MyUtils.py:25      Div0(0, 0)                               */
#define RR_STATUS_STEP_AFTER_DONE 64   /* RR_EnvBase.py:262  "Game is over" (auto_reset = 0 only)     */
#define RR_STATUS_BAD_ACTION 128       /* action outside 0..7 (KeyError in RR_EnvBase.py:606)         */
#define RR_STATUS_UNDO_WARN 256        /* RR_EnvBase.py:419  GAME_MODE warning, step continued        */
#define RR_STATUS_RESET_GAVE_UP 512    /* spawn rejection sampling hit its attempt cap                */
#define RR_STATUS_WAS_RESET 1024       /* this call reset the arena instead of stepping it            */
#define RR_STATUS_NOT_READY 16384       /* budgeted step only: this arena's step is still in progress (see step_budget_clocks) */
#define RR_STATUS_FLAG_MASK 0xFFFF     /* bits 0-15 are the flags above ...                            */
#define RR_STATUS_NAUGHTY_SHIFT 16     /* ... bits 16+r: robot r joined NaughtyBots' set this step (RR_ScoreKeepers.py:123-128) */

#define RR_DTYPE_F64 0 /* state + arithmetic in fp64: the parity mode (the reference is fp64)         */
#define RR_DTYPE_F32 1 /* state + arithmetic in fp32: the fast mode                                   */
#define RR_DTYPE_F32_STATE 2 /* "fp32 state" (BASELINE config 2): the arenas' records in HBM are fp32, a step computes in fp64 between
                                loading a record and writing it back -- one rounding per stored value and step, single-step results
                                within 1e-5 of the fp64 reference on contact steps too.  The shape's lane width, rr_step / rr_step_f64 /
                                rr_step_thrust(_f64) and every side entry; no rr_rollout, no step budget (both would keep unrounded
                                state across steps) */

#define RR_TEAM_HAPPY 1   /* RR_Constants.py:52 */
#define RR_TEAM_GRUMPY (-1) /* RR_Constants.py:53 */

#define RR_OBS_DIM 11 /* SingleBall_6wayLidar_v2, RR_Observers.py:394-406 */

typedef struct rr_env rr_env; /* opaque */

typedef struct rr_config {
    int32_t struct_size;    /* = sizeof(rr_config), for forward compatibility                          */
    int32_t num_envs;       /* N arenas stepped in lockstep by this handle                             */
    int32_t nr_happy, nr_grumpy, nb_pos, nb_neg; /* RR_Constants.py:30-34; shapes inside libroborugby_amd.so: (1,0,1,0), (2,2,4,4), (1,1,1,1);
                                                    any other counts (<= 8 robots, <= 11 balls, <= 32 ball-robot pairs): a one-shape library of the same
                                                    sources and ABI, hipcc -DRR_CUSTOM_SHAPE ... (roborugby_amd/build.py: build_shape_library) */
    double arena_w, arena_h;                     /* RR_Constants.py:6-7: the two are independent, each in [300, 8192].  Pass INTEGERS, as the
                                                    reference's are (its reset draws positions with random.randint over them; the kernel
                                                    truncates).  Pinned to reference vectors: 800 x 800, 600 x 600, and the non-square
                                                    1000 x 640 and 480 x 720 (tests/golden: traj / reset _Dwide, _Ttall).  A ball beyond the bottom wall
                                                    is reflected with H - (bottom - W) * 1.1 -- the WIDTH, as RR_TrashyPhysics.py:336 has it:
                                                    kept on purpose, it only shows when W != H                                          */
    int32_t game_len_steps; /* RR_Constants.py:25                                                      */
    int32_t game_mode;      /* RR_Constants.py:4: only selects the undo-loop fault rule (EnvBase:417-421) */
    int32_t time_limit;     /* 1: done = step_count >= T (what gym's TimeLimit wrapper reports to
                               Training_DQN_pytorch.py); 0: done = step_count > T (raw RR_EnvBase.py:555-559) */
    int32_t auto_reset;     /* 1: rr_step on a finished arena resets it (status WAS_RESET, reward 0, done 0)
                               instead of flagging STEP_AFTER_DONE                                     */
    int32_t reset_on_fault; /* 1: a step that ends with a fatal status (the places where the reference raises or
                               spins forever: bits 1|2|4|8|16|32) reports done = 1 and ends the episode, so that
                               auto_reset re-places the arena; 0: the arena keeps stepping with the bit set     */
    int32_t dtype;          /* RR_DTYPE_F64 | RR_DTYPE_F32 | RR_DTYPE_F32_STATE                        */
    int32_t device;         /* HIP device ordinal                                                      */
    uint64_t seed;          /* keys the counter-based reset RNG                                        */
    uint64_t arena_offset;  /* global id of local arena 0: makes results invariant to sharding         */
    uint32_t step_budget_clocks; /* 0 (default): every rr_step call completes every arena's step -- the reference's semantics
                               (RR_EnvBase.py:260-297), and the call lasts as long as its slowest arena.  > 0: the BUDGETED step,
                               an opt-in extension for contact-rich policies: an arena whose wavefront has run for more than this
                               many shader clocks at the end of an expensive physics sub-step (RR_EnvBase.py:275-287 runs 12 per
                               step) parks there; the call reports RR_STATUS_NOT_READY for it -- reward 0, done 0, its obs / obs_g
                               rows NOT written (reuse the buffers to keep the previous ones) -- and the next call resumes it where
                               it stopped, IGNORING the action it is given.  Each arena's trajectory as a function of the actions
                               it accepted is bit-identical to step_budget_clocks = 0.  Works with every reward program, observer, prior-step
                               tracking and the goal-scoring mode: their side kernels take the on_step_begin copies when an arena's step
                               BEGINS and run its on_step_end with the call that completes it (switch prior-step tracking on before the
                               budget, or after a call without NOT_READY rows). */
    uint32_t reserved_;     /* 0                                                                       */
} rr_config;

int rr_abi_version(void);
/* 1 in the parity build (libroborugby_amd_exact.so: the same sources with -DRR_EXACT_TRIG=1), 0 in the default library.  The parity
 * build (a) evaluates sin / cos of the robot kinematics in double-double, ~correctly rounded, so that they agree with the reference's
 * math.sin / math.cos (glibc) on 99.85 % of the evaluations instead of 97 %, and (b) carries the centre of the reference's scratch rect
 * (rr_get/set_scratch_rect below): free-running episodes then follow the reference bit for bit -- most of them to their last step --
 * at ~80 % of the default library's speed. */
int rr_exact_trig(void);
const char *rr_last_error(void); /* thread-local description of the last <0 return */

/* Allocates the per-arena state (SoA records in HBM) on cfg->device and places every arena like the
 * reference constructor does (RR_EnvBase.py:111-116 -> _set_random_positions). */
int rr_create(const rr_config *cfg, rr_env **out);
int rr_destroy(rr_env *env);

/* env.reset() (RR_EnvBase.py:202-216) for the arenas whose mask byte is non-zero (mask == NULL: all).
 * obs [N,11] float32, obs_g [N,11] float32 (nullable; NaN rows when there is no grumpy robot). */
int rr_reset(rr_env *env, const uint8_t *mask, float *obs, float *obs_g, void *stream);

/* GameEnv_Simple.step (RR_EnvBase.py:617-626 -> :260-297): actions [N,na] int32 in 0..7, action i
 * drives robot i (happy robots first); robots without an action keep their thrust.  Outputs (all
 * nullable except obs/reward/done): obs [N,11] f32, reward [N] f32, done [N] u8, obs_g [N,11] f32,
 * reward_g [N] f32 (info.adblGrumpyState / info.dblGrumpyScore, RR_EnvBase.py:562-566),
 * status [N] i32. */
int rr_step(rr_env *env, const int32_t *actions, int32_t na, float *obs, float *reward, uint8_t *done,
            float *obs_g, float *reward_g, int32_t *status, void *stream);
/* Same step with fp64 outputs (full-precision parity checks). */
int rr_step_f64(rr_env *env, const int32_t *actions, int32_t na, double *obs, double *reward, uint8_t *done,
                double *obs_g, double *reward_g, int32_t *status, void *stream);
/* Changes rr_config.step_budget_clocks of a live handle (host-side; takes effect with the next rr_step).  0 switches parking
 * off -- arenas that are parked at that moment finish their step in the next call(s) as usual.  Any value may be set while
 * arenas are parked: they go on with their step under the new budget; their observation rows are not touched. */
int rr_set_step_budget(rr_env *env, uint32_t clocks);
/* Open-loop rollout: nsteps consecutive rr_step calls per arena in ONE launch -- the record stays in LDS, and no arena
 * waits for the slowest arena of the batch between steps (a launch per step ends when its slowest wavefront does).
 * actions [nsteps, N, na] (repeat == 0) or [N, na] applied at every step (repeat != 0: the action-repeat / frame-skip
 * wrapper of RL practice); outputs are stacked per step: obs [nsteps, N, 11], reward / done / status [nsteps, N]
 * (obs_g, reward_g, status nullable).  Bit-identical to calling rr_step nsteps times (auto-reset included).  The reference
 * has no counterpart (gym steps one call at a time); policies that need step s's observation to choose step s+1's
 * action use rr_step. */
int rr_rollout(rr_env *env, const int32_t *actions, int32_t na, int32_t nsteps, int32_t repeat, float *obs, float *reward,
               uint8_t *done, float *obs_g, float *reward_g, int32_t *status, void *stream);

/* Continuous entry, GameEnv.step (RR_EnvBase.py:260-273): thrust [N,2*nk] float32 (L,R per robot),
 * rounded half-to-even like Python's round() (RR_Robot.py:100-102). */
int rr_step_thrust(rr_env *env, const float *thrust, int32_t nk, float *obs, float *reward, uint8_t *done,
                   float *obs_g, float *reward_g, int32_t *status, void *stream);
/* Same entry with fp64 outputs (the thrust entry's observation / reward parity checks; RR_DTYPE_F64 / RR_DTYPE_F32_STATE handles only). */
int rr_step_thrust_f64(rr_env *env, const float *thrust, int32_t nk, double *obs, double *reward, uint8_t *done,
                       double *obs_g, double *reward_g, int32_t *status, void *stream);

/* get_game_state(int_team=team) (RR_Observers.py:301-406) of the current state; robot_idx/ball_idx
 * = -1 selects the team's first robot / positive ball 0 like the reference defaults. */
int rr_observe(rr_env *env, int32_t team, int32_t robot_idx, int32_t ball_idx, float *obs, void *stream);
int rr_observe_f64(rr_env *env, int32_t team, int32_t robot_idx, int32_t ball_idx, double *obs, void *stream);

/* Full state exchange in the canonical fp64 layout (same as tests/golden/traj_*.npz):
 *   robots   [N,NR,10] cx,cy,left,right,top,bottom,rot,prev_x,prev_y,prev_rot (prev = pose ring entry
 *            moveCount-1, RR_Robot.py:43-58; NaN = absent)
 *   robots_i [N,NR,3]  moveCount,lthrust,rthrust
 *   balls    [N,NB,8]  cx,cy,left,right,top,bottom,vx,vy
 *   step     [N]       lngStepCount */
int rr_set_state(rr_env *env, const double *robots, const int32_t *robots_i, const double *balls,
                 const int32_t *step, void *stream);
int rr_get_state(rr_env *env, double *robots, int32_t *robots_i, double *balls, int32_t *step, void *stream);
/* Poses only -- the reference's lst_starting_config format (RR_EnvBase.py:35-52,131-153) plus ball
 * velocities: robots_xyr [N,NR,3], balls_xyv [N,NB,4]; edges re-derived, history cleared. */
int rr_set_poses(rr_env *env, const double *robots_xyr, const double *balls_xyv, void *stream);
/* env.reset(bln_randomize_pos=False) (RR_EnvBase.py:202-216 -> _set_starting_positions :131-153): the arenas whose mask
 * byte is non-zero (mask == NULL: all) restart at the given start configuration -- robots_xyr [N,NR,3], balls_xyv [N,NB,4]
 * (the reference's lst_starting_config, zero ball velocities) -- with step count 0, thrust 0, no pose history; obs / obs_g
 * (nullable) receive the first observations of the masked arenas.  The caller keeps the layout (the Python mirror retains
 * the construction placement exactly like GameEnv.__init__ keeps self._lst_starting_positions, RR_EnvBase.py:111-116). */
int rr_reset_to_poses(rr_env *env, const uint8_t *mask, const double *robots_xyr, const double *balls_xyv, float *obs,
                      float *obs_g, void *stream);
/* Episode bookkeeping for checkpoint / resume (build-side; the reference pickles the agent and never the env):
 * ints [N,5] = episode index (keys the reset RNG), steps in the running episode, finished episodes, length of the last
 * finished episode, fault flag; acc [N,4] = running return happy / grumpy, last finished return happy / grumpy. */
/* Parity build only (rr_exact_trig() == 1; the default library returns -3): the centre of the reference's module-global scratch
 * rect `_rectBallInner` (RR_TrashyPhysics.py:26-36), xy [N,2] fp64, device pointers.  Its centre setters are relative moves
 * (MyUtils.py:266-275), so the centre the next ball diameter is built from depends, in the last bits, on where the previous user left
 * it -- state that survives resets and, in a process that runs several envs, episodes.  The parity build keeps it in each arena's
 * record; rr_set_state puts it on the last ball (where every sub-step leaves it), rr_set_scratch_rect seeds it from a dumped
 * reference state (tests/golden/traj_*.npz `state_inner`), rr_reset / rr_set_poses leave it alone like the reference does. */
int rr_get_scratch_rect(rr_env *env, double *xy, void *stream);
int rr_set_scratch_rect(rr_env *env, const double *xy, void *stream);
int rr_get_episode_state(rr_env *env, int32_t *ints, double *acc, void *stream);
int rr_set_episode_state(rr_env *env, const int32_t *ints, const double *acc, void *stream);

/* ---- the reference's other mixins; SimpleDuel3's own stack is the default and is fused
 * into the step kernel, anything else is evaluated by light side kernels around it.
 * Reward keepers, given in on_step_end EXECUTION order (each keeper calls super() first, except NaughtyBots which
 * never does, so keepers behind it in the MRO do not run): 1 NaughtyBots, 2 ChasePosBall, 3 PushPosBallsToGoal,
 * 4 DontDriveInGoals, 5 KeepMovingGuys, 6 BaseDestruction, 7 PushNegBallsFromGoal (RR_ScoreKeepers.py:46-179).
 * Default {1,2,3}.  n <= 8.
 * Budgeted step: a switch takes effect with the steps that complete from the next call on -- a parked arena's step is scored by
 * the new program from the on_step_begin copies taken when that step began.  Those copies are only kept while a non-default
 * program or rr_track_prior_step is on: a switch from the default program with tracking off, while some arena is parked, returns
 * -1 and changes nothing (rr_set_step_budget(env, 0) and one rr_step first: no arena is parked then). */
int rr_set_reward_program(rr_env *env, const int32_t *keeper_ids, int32_t n);
/* Observers: kind 0 SingleBall_6wayLidar_v2 (11 values), 1 SingleBall_6wayLidar (11, RR_Observers.py:168-285),
 * 2 PosBall_BasicLidar (5, :116-166), 3 AllCoords (3*NR + 2*NB, :47-83), 4 AllCoords_WithPrior (6*NR + 4*NB, :86-110:
 * every robot x, y, rot + its rectDblPriorStep x, y, rot, every ball x, y + prior-step x, y; needs
 * rr_track_prior_step).  obs [N, out_dim]; rows are NaN where the reference returns None.  out_dim must equal the
 * kind's size. */
int rr_observe_kind(rr_env *env, int32_t kind, int32_t team, int32_t robot_idx, int32_t ball_idx, float *obs,
                    int32_t out_dim, void *stream);
int rr_observe_kind_f64(rr_env *env, int32_t kind, int32_t team, int32_t robot_idx, int32_t ball_idx, double *obs,
                        int32_t out_dim, void *stream);

/* The hive-mind player's view -- Stephen.__ponder + the observation Stephen.__consult asks for (DQN_pytorch_player.py:38-71) -- for
 * every arena in ONE launch: which ball each hive robot goes for, and get_game_state(obj_robot = that robot, obj_ball = that ball).
 * robot_mask: bit r set = robot r (happy robots first) belongs to the hive; robots of both teams may be in it and then compete for
 *             balls in the same greedy pass, as the reference's class-level hive does.  Empty, or a bit >= NR: -1.
 * kind:       0 SingleBall_6wayLidar_v2 | 1 SingleBall_6wayLidar (the one Stephen insists on); others: -1.
 * assign [N,NR] i32: ball index (positive balls first) given to robot r, -1 = none (also for robots outside the hive).
 * obs [N,NR,11]:     what rr_observe_kind(kind, team of r, r, assign) returns, including the flip for a negative ball / grumpy
 *                    robot; rows with assign -1 are 0.
 * Assignment: candidate balls are those whose centre is in neither goal triangle (Goal.ball_in_goal, RR_Goal.py:71) and, with the
 * opt-in goal scoring, still in play; the (robot, ball) pairs are walked by ascending MyUtils.distance of the two centres, a pair is
 * taken when neither its robot nor its ball is taken yet.  Distances are compared in the handle's arithmetic type (fp32 for
 * RR_DTYPE_F32, else fp64).  TIES: the reference does not define the order of exactly equal distances (it iterates a Python set of
 * players); here the pair with the lower ball index goes first, then the one with the lower robot index.
 * Read-only on the records: callable between any two steps and changes no later step.  On a handle with a step budget the record
 * of a parked arena (RR_STATUS_NOT_READY) is in the middle of its step: its row is a sub-step view; the step ignores the action
 * given to such an arena anyway.  rr_hive_observe_f64 refuses RR_DTYPE_F32 like rr_observe_f64. */
int rr_hive_observe(rr_env *env, uint32_t robot_mask, int32_t kind, int32_t *assign, float *obs, void *stream);
int rr_hive_observe_f64(rr_env *env, uint32_t robot_mask, int32_t kind, int32_t *assign, double *obs, void *stream);

/* on != 0: every rr_step / rr_step_thrust first snapshots what the sprites' on_step_begin copies (rectDblPriorStep,
 * RR_Robot.py:116-117, RR_Ball.py:60-61) so that observer kind 4 can report it; the call itself (and rr_reset) seeds the
 * copies from the current poses (the reference holds the stale pre-placement pose until the first step).
 * Budgeted step: a parked arena keeps the copies of its step begin.  Switching on while the default keeper program is set and some
 * arena is parked returns -1 and changes nothing -- no copies were kept when those steps began (see rr_set_reward_program). */
int rr_track_prior_step(rr_env *env, int32_t on, void *stream);

/* Training the hive in the full game: the transition of every hive robot over the step that was just taken, in ONE launch.  Call order:
 * rr_track_prior_step(env, 1) once; then per step rr_hive_observe (assign, obs) -> rr_step* (status, done) -> this.
 * assign [N,NR] i32:  what rr_hive_observe wrote BEFORE the step.  status [N] i32, done [N] u8: the step's.
 * Row (a, r) is VALID when r is in robot_mask, 0 <= assign[a,r] < NB (any other value, garbage included, makes the row invalid and is
 * never used as an index), the step's status has none of RR_STATUS_WAS_RESET / NOT_READY / STEP_AFTER_DONE, and the ball is still in
 * play (opt-in goal scoring: a ball consumed during this step ends the pairing without a transition).  For a valid row
 *   next_obs [N,NR,11]: what rr_observe_kind(kind, team of r, r, assign[a,r]) returns on the record after the step -- the ball is held,
 *                       not re-assigned, even if it now lies in a goal;
 *   reward [N,NR]:      the reference has no per-robot reward; this is SimpleDuel3's three keepers restricted to the pair, summed in the
 *                       handle's arithmetic type from 0 in this order: (1) NaughtyBots: -0.005 if status bit 16 + r is set;
 *                       (2) ChasePosBall: (dist(prior_r, ball_now) - dist(robot_now, ball_now)) * mult_robot, prior_r the robot's
 *                       on_step_begin copy, ball_now the ball's centre after the step in both distances; (3) PushPosBallsToGoal:
 *                       sgn * (dist((0,0), ball_now) - dist((0,0), ball_prior)) * mult_ball, ball_prior the ball's on_step_begin copy,
 *                       sgn = (r happy ? +1 : -1) * (ball positive ? +1 : -1) -- negative for exactly the pairs whose observation is
 *                       turned round.  dist is MyUtils.distance as the reference evaluates it, ((bx-ax)**2 + (by-ay)**2)**.5 with
 *                       both powers through pow().  With one robot per team and positive ball 0 the sum is the team's reward: the
 *                       reference's own bit for bit where pow is the host libm's, rr_step's within a few 1e-11 on the device;
 *   terminal [N,NR] u8: done[a].
 * Invalid rows: next_obs 0, reward 0, terminal 0, valid [N,NR] u8 0.  Every output element is written on every call.
 * Returns -1 (message in rr_last_error, nothing launched): null handle / pointer; empty mask or a mask bit >= NR; kind not 0 or 1;
 * prior-step tracking off; a handle that has (had) a step budget -- a parked arena's pre-step assignment is overwritten by the next
 * rr_hive_observe before its step completes (rr_hive_transition_held below is the entry for such a handle).  Read-only on the records and the snapshot.  rr_hive_transition_f64 refuses RR_DTYPE_F32
 * like rr_hive_observe_f64. */
int rr_hive_transition(rr_env *env, uint32_t robot_mask, int32_t kind, const int32_t *assign, const int32_t *status, const uint8_t *done,
                       float *next_obs, float *reward, uint8_t *terminal, uint8_t *valid, void *stream);
int rr_hive_transition_f64(rr_env *env, uint32_t robot_mask, int32_t kind, const int32_t *assign, const int32_t *status, const uint8_t *done,
                           double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid, void *stream);

/* The hive under the budgeted step: HELD ROWS.  On a handle with a step budget an arena's step may span several calls; the transition it
 * completes belongs to the assignment it was given, the observation the agent was asked on and the action it answered before the step
 * began.  These entries keep those three rows while the arena is parked.  Call order per step, all with the SAME assign, obs and
 * accepted buffers:
 *   rr_hive_observe_held -> rr_dqn_act (into a scratch `fresh`) -> rr_hive_commit -> rr_step_thrust -> rr_hive_transition_held
 * Then (obs, accepted, reward, next_obs, terminal) of a valid row is the transition of the step the arena accepted, however many calls
 * that step took, and each arena's stream of such transitions is the synchronous mode's bit for bit.
 *
 * rr_hive_observe_held: rr_hive_observe, except that an arena parked mid-step gets held[a] = 1 and its assign / obs rows are NOT
 *   written; every other arena gets held[a] = 0 and the rows rr_hive_observe writes.  held [N] u8, required.  The parked mark is read
 *   from the arena's record, not from a status: a reset / rr_set_state / rr_set_poses of a parked arena clears it and the arena is
 *   observed afresh.  On a handle that never had a budget: rr_hive_observe with held all 0.
 * rr_hive_commit: the tail of the hive's turn.  fresh [N,NR] i32: the agent's answers to obs (rr_dqn_act); assign, held: as written
 *   above.  For an arena that is not held and every robot r in robot_mask: accepted[a,r] = fresh[a,r], and thrust[a, 2r .. 2r+1] =
 *   _dct_thrust_from_direction[fresh[a,r]] (RR_EnvBase.py:593-602) when assign[a,r] >= 0 and 0 <= fresh[a,r] < 8, else (0, 0) -- an
 *   out-of-range value is never an index.  Nothing of a held arena is written (the step ignores its thrust), nor the columns of robots
 *   outside the mask (another player drives them).  accepted [N,NR] i32, thrust [N,2*NR] f32.
 * rr_hive_transition_held: rr_hive_transition -- same rows, bit for bit -- that is accepted on a handle with a step budget; an arena
 *   that did not step (RR_STATUS_NOT_READY among them) is an invalid row and is written without reading its record.
 * Guards as on rr_hive_observe / rr_hive_transition (-1, message in rr_last_error, nothing launched); launch-only: no allocation, no
 * synchronisation.  The _f64 entries refuse RR_DTYPE_F32. */
int rr_hive_observe_held(rr_env *env, uint32_t robot_mask, int32_t kind, int32_t *assign, float *obs, uint8_t *held, void *stream);
int rr_hive_observe_held_f64(rr_env *env, uint32_t robot_mask, int32_t kind, int32_t *assign, double *obs, uint8_t *held, void *stream);
int rr_hive_commit(rr_env *env, uint32_t robot_mask, const int32_t *fresh, const int32_t *assign, const uint8_t *held, int32_t *accepted,
                   float *thrust, void *stream);
int rr_hive_transition_held(rr_env *env, uint32_t robot_mask, int32_t kind, const int32_t *assign, const int32_t *status,
                            const uint8_t *done, float *next_obs, float *reward, uint8_t *terminal, uint8_t *valid, void *stream);
int rr_hive_transition_held_f64(rr_env *env, uint32_t robot_mask, int32_t kind, const int32_t *assign, const int32_t *status,
                                const uint8_t *done, double *next_obs, double *reward, uint8_t *terminal, uint8_t *valid, void *stream);

/* Opt-in goal scoring -- an EXTENSION: on the reference's live path the goals never score (Goal.track_balls / update_score are
 * only reached from the never-called GameEnv.__old_step, RR_EnvBase.py:458-520; RR_Goal.py:80 calls a property as a function),
 * so there is no reference behaviour to match; this is the mechanism of RR_Goal.py:54-91 + the commented block at
 * RR_EnvBase.py:494-512 made to work as SURVEY 8(f)-3 words the intent: a ball inside a goal triangle for 150 consecutive steps
 * is consumed (out of play from then on: parked at x <= -1000), +-500 points (happy team +500 for a positive ball in the happy
 * goal / a negative one in the grumpy goal, the grumpy team the opposite), 3 negative balls destroy a goal, and a destroyed goal
 * or an empty field ends the episode (done = 1, status bits below; BaseDestruction pays when it is in the keeper program).
 * Ordering: the step that consumes a ball still OBSERVES it inside the goal (the goal bookkeeping runs after the step's
 * observation is taken); the ball is out of play from the next observation on.
 * rr_goal_scores: Goal.get_score() of (happy, grumpy) goal per arena, int32 [N,2]; all zero while the mode is off. */
#define RR_STATUS_GOAL_H_DESTROYED 2048
#define RR_STATUS_GOAL_G_DESTROYED 4096
#define RR_STATUS_NO_BALLS 8192
int rr_set_goal_scoring(rr_env *env, int32_t on, void *stream);
int rr_goal_scores(rr_env *env, int32_t *scores, void *stream);

/* Logging: return/length of the last finished episode and the number of finished episodes per arena
 * (the caller accumulates `score` the same way, Training_DQN_pytorch.py:345-346). */
int rr_episode_stats(rr_env *env, float *last_return, float *last_return_g, int32_t *last_len,
                     int32_t *episodes_done, void *stream);

/* Scripted on-device policy of the contact-rich benchmark stream (the reference's scripted players
 * live in robo_rugby/gym_env/RR_Players.py): robot 0 of every arena turns toward its ball (observation values 0 and 1:
 * bot angle, ball angle) or drives forward when within 8 degrees, and with probability `noise` takes a random action; robots
 * 1..na-1 act at random.  obs [N,11] f32 (the rows rr_step / rr_reset wrote), actions [N,na] i32.  The random draws are a
 * function of (seed, global arena id, step index) only; the step index is step_of[arena] when step_of != NULL (per-arena
 * counters, e.g. "steps accepted so far" under the budgeted step), else `step`.  One launch, nothing else. */
int rr_policy_chase(rr_env *env, const float *obs, const int32_t *step_of, uint32_t step, float noise, uint64_t seed,
                    int32_t *actions, int32_t na, void *stream);

/* Pictures: RGB frames of many arenas in one launch, straight from the records (csrc/rr_render.hpp).  What render() draws on the host
 * for one arena -- goals, robots, balls, in the colours of roborugby_amd/render.py -- without the dashboard strip, at any size: small
 * enough to tile a running batch into a contact sheet, or to serve as a pixel observation.  An extension (the reference draws with pygame).
 *
 * The picture.  Arena coordinates, y down.  A frame shows the field only (W x H), scaled independently in x and y to width x height
 * pixels, with S = `samples` (1, 2 or 4) samples per axis and pixel.  Sample (a, b) of pixel (i, j) is the point
 *     x = ((float)(i*S + a) + 0.5f) * fx,   y = ((float)(j*S + b) + 0.5f) * fy,
 *     fx = (float)(W / (double)(width*S)),  fy = (float)(H / (double)(height*S))        (fx, fy computed once on the host)
 * -- a frame with S samples at `width` decides the same sample points as a frame with 1 sample at width*S.  A sample takes the colour of
 * the topmost layer that contains it; boundaries are closed; all arithmetic is fp32 (a record's fp64 values are rounded first):
 *   1. background (255, 255, 255);
 *   2. goals (RR_Goal.py:14-28, 240 = GOAL_WIDTH): grumpy (242, 53, 87) where x + y <= 240; happy (43, 146, 228) where
 *      (W - x) + (H - y) <= 240;
 *   3. robots 0 .. NR-1, a later one over an earlier one.  th = radians(360 - rot), c = cos th, s = sin th, (dx, dy) = sample - centre,
 *      u = dx*c + dy*s, v = -dx*s + dy*c (the inverse of render.robot_corners).  Inside: |u| <= 10 && |v| <= 20 -- the rectangle the
 *      collision geometry uses.  Black (0, 0, 0) where |u| > 9 || |v| > 19; else yellow (255, 255, 0) where u > 7 (the front is the
 *      RIGHT side, RR_Observers.py:322-324); else the team colour, (40, 90, 200) for robots below nr_happy, (200, 60, 60) for the others;
 *   4. balls 0 .. NB-1, later over earlier.  Inside: dx*dx + dy*dy <= 49; black where > 36, else (80, 220, 100) for positive balls and
 *      (60, 16, 83) for negative ones.
 * An entity with a non-finite pose draws nothing; a ball consumed by goal scoring is parked at x <= -1000 and falls outside the frame by
 * itself.  With S > 1 each channel is (sum of the S*S sample values + S*S/2) / (S*S) in integer arithmetic.  A frame whose arena index
 * is outside 0 .. N-1 is written all zero (black, which no in-range frame of a white field is); such an index is never used as an index.
 *
 * arenas [m] i32 DEVICE pointer, NULL = arenas 0 .. m-1; duplicates and any order are allowed.  rgb [m, height, width, 3] u8, 4-byte
 * aligned: every byte of the m frames is written on every call, and nothing beyond them.  Read-only on the records; accepted on every
 * handle -- all three dtypes, both libraries and the one-shape libraries, and handles with a step budget: an arena parked mid-step shows
 * its mid-step record, as rr_hive_observe does.  Returns -1 (rr_last_error) and launches nothing for a null handle or rgb, m outside
 * 1 .. 1 << 20, width outside 4 .. 4096 or not a multiple of 4, height outside 1 .. 4096, samples not 1, 2 or 4, or a misaligned rgb.
 * Launch-only: no allocation, no synchronisation (more than 65,535 frames go out as several launches on the same stream). */
int rr_render(rr_env *env, const int32_t *arenas, int32_t m, int32_t width, int32_t height, int32_t samples,
              uint8_t *rgb, void *stream);

/* Egocentric pictures: one frame per (arena, robot), centred on the robot, its front up, coloured from its own side -- what a policy
 * that drives ONE robot can look at (rr_render's frames are absolute in place, direction and team colour).  csrc/rr_render.hpp:
 * k_render_ego.  An extension.
 *
 * Which arena and robot a frame shows.  Frame k shows arena arenas[k] (arenas == NULL: arena k) seen from robot robots[k], happy robots
 * first (robots == NULL: robot 0).  Both are DEVICE pointers; duplicates and any order are allowed.
 *
 * Camera.  (cx, cy, rot) is the viewing robot's pose from the record, rounded to fp32; th = (360 - rot) * 0.017453292519943295f,
 * c = cosf(th), s = sinf(th) -- exactly the values the draw list of rr_render holds for that robot.  The robot's front is its +u side
 * (rr_render's convention); the front points UP in the frame, frame-right is the robot's +v side.
 *
 * Sample points.  All arithmetic is fp32; the three view constants are computed once on the host in double and then rounded:
 *     f = (float)(span / (double)(width*S)),  hx = (float)(span * 0.5),  hy = (float)(span * 0.5 * height / width).
 * Sample (a, b) of pixel (i, j), with S = `samples`, is
 *     p = ((float)(i*S + a) + 0.5f) * f - hx          (to the right)
 *     q = ((float)(j*S + b) + 0.5f) * f - hy          (downwards)
 *     fwd = ahead - q
 *     x = cx + (fwd*c - p*s),   y = cy + (fwd*s + p*c)
 * The frame covers `span` arena units across and span*height/width down, both axes at the same scale; the robot's centre sits `ahead`
 * units below the frame's centre (ahead > 0 looks further forward).  A frame with S samples at `width` decides the same sample points as
 * a frame with 1 sample at width*S.
 *
 * Layers at (x, y): exactly rr_render's 1-4 -- background, goals, robots 0 .. NR-1, balls 0 .. NB-1, closed boundaries, the same inside
 * tests; the viewing robot is drawn like any other -- and one new layer ON TOP: a sample with x < 0 || x > W || y < 0 || y > H is
 * OUTSIDE, (96, 96, 96).  So the walls are visible, and a ball parked at x <= -1000 by goal scoring never shows.
 *
 * Colours with RR_EGO_RELATIVE: if the viewing robot is grumpy (index >= nr_happy) the palette is swapped pairwise -- the two team
 * colours, the two ball colours, the two goal colours: blue robots and the blue goal are "mine", the green ball is "the one that scores
 * for me", for either team.  For a happy viewer, or without the flag, the colours are rr_render's.
 *
 * The box filter for S > 1 is rr_render's.  rgb is [m, height, width, 3], with RR_EGO_PLANAR [m, 3, height, width]; every byte of the m
 * frames is written on every call, and nothing beyond them.  A frame is written all zero if its arena index is outside 0 .. N-1, its
 * robot index is outside 0 .. NR-1, or the viewing robot's pose is non-finite; such a value is never used as an index.
 *
 * Returns -1 (rr_last_error, "rr_render_ego: ...") and launches nothing for a null handle or rgb, m outside 1 .. 1 << 20, width outside
 * 4 .. 1024 or not a multiple of 4, height outside 1 .. 1024, samples not 1, 2 or 4, span not finite or outside 16 .. 16384, ahead not
 * finite or |ahead| > 8192, flag bits other than the two above, or an rgb that is not 4-byte aligned.  Accepted on every handle
 * rr_render accepts (all dtypes, both libraries, one-shape libraries, budgeted handles: a parked arena shows its mid-step record);
 * read-only on the records; launch-only: no allocation, no synchronisation. */
#define RR_EGO_RELATIVE 1  /* colours from the viewing robot's side */
#define RR_EGO_PLANAR   2  /* rgb is [m,3,height,width] instead of [m,height,width,3] */
int rr_render_ego(rr_env *env, const int32_t *arenas, const int32_t *robots, int32_t m, int32_t width, int32_t height,
                  int32_t samples, float span, float ahead, int32_t flags, uint8_t *rgb, void *stream);

/* ---- config 5 (BASELINE.json): the learn step of the reference's DQN agent (Training_DQN_pytorch.py:25-67 DeepQNetwork
 * Linear 11 -> 256 -> 256 -> 8 + ReLU, MSELoss, Adam; :151-191 DQNAgent.learn) fused into two launches for the wide batches of the
 * batched trainer: forward of Q_eval(s) and Q_target(s'), TD target, loss gradient, backward and the weight-gradient reduction in
 * one kernel (fp32 matrix cores, activations resident in LDS), partial-gradient reduction + Adam in the second
 * (roborugby_amd/csrc/rr_dqn.hip).  Every pointer is a device pointer; the parameters stay PyTorch's (updated in place), the
 * handle owns the Adam moments and the scratch.  Same math as torch autograd up to fp32 summation order. */
typedef struct rr_dqn rr_dqn; /* opaque */
typedef struct rr_dqn_args {
    int32_t struct_size;            /* = sizeof(rr_dqn_args) */
    int32_t batch;                  /* samples per update: a positive multiple of 64 */
    float *eval_params[6];          /* fc1.weight [256,11], fc1.bias [256], fc2.weight [256,256], fc2.bias [256], fc3.weight [8,256],
                                       fc3.bias [8] of Q_eval (row-major, torch.nn.Linear layout): updated in place */
    const float *target_params[6];  /* the same six tensors of Q_target */
    const float *state_memory;      /* replay memory (Training_DQN_pytorch.py:95-104): [M,11] */
    const float *new_state_memory;  /* [M,11] */
    const int64_t *action_memory;   /* [M] */
    const float *reward_memory;     /* [M] */
    const uint8_t *terminal_memory; /* [M] (torch.bool) */
    const int64_t *batch_index;     /* [batch] sampled rows of the memory (NULL: rows 0 .. batch-1) */
    float gamma, lr, beta1, beta2, eps; /* :79 gamma; torch.optim.Adam defaults 1e-3 / .9 / .999 / 1e-8 unless set (:42 lr) */
    float *loss_out;                /* nullable: the batch's mean squared TD error (MSELoss) */
} rr_dqn_args;
int rr_dqn_create(int32_t device, rr_dqn **out);
int rr_dqn_destroy(rr_dqn *dqn);
const char *rr_dqn_last_error(void);
/* One gradient step: Q_eval's parameters <- Adam(grad of MSE(r + gamma max_a' Q_target(s'), Q_eval(s)[a])). */
int rr_dqn_update(rr_dqn *dqn, const rr_dqn_args *args, void *stream);
/* The same gradient without the update: grads [rr_dqn_param_count()] in the order fc2.weight, fc1.weight, fc3.weight, fc1.bias,
 * fc2.bias, fc3.bias (the parity tests' window). */
int rr_dqn_grads(rr_dqn *dqn, const rr_dqn_args *args, float *grads, void *stream);
int32_t rr_dqn_param_count(void);
/* DQNAgent.choose_action (Training_DQN_pytorch.py:138-149) for n observations (a multiple of 64) in one launch: actions[i] =
 * argmax_a Q(obs[i]) (first maximum), or with probability epsilon a uniform action -- the draw is a function of (seed, i, call),
 * so pass a fresh `call` counter every time.  params = the six tensors of the network to act with (rr_dqn_args.eval_params
 * order); qvalues [n,8] is optional (NULL: not written). */
int rr_dqn_act(rr_dqn *dqn, const float *const params[6], const float *obs, int32_t n, float epsilon, uint64_t seed, uint32_t call,
               int32_t *actions, float *qvalues, void *stream);
/* DQNAgent.store_transition (Training_DQN_pytorch.py:126-136) for n transitions in one launch: the rows whose `valid` byte is set
 * (NULL: all) are appended to the replay ring at mem_cntr, mem_cntr + 1, ... (mod mem_size) in row order; count_out (device int32,
 * nullable) receives how many.  state / new_state [n,11] f32, action [n] i32, reward [n] f32, done [n] u8 (torch.bool). */
int rr_dqn_store(rr_dqn *dqn, const float *state, const int32_t *action, const float *reward, const float *new_state,
                 const uint8_t *done, const uint8_t *valid, int32_t n, int64_t mem_cntr, int64_t mem_size, float *state_memory,
                 float *new_state_memory, int64_t *action_memory, float *reward_memory, uint8_t *terminal_memory,
                 int32_t *count_out, void *stream);
/* Adam moments (same order as rr_dqn_grads) and step count out of / into the handle: checkpoint / resume. */
int rr_dqn_adam_state(rr_dqn *dqn, float *exp_avg, float *exp_avg_sq, int64_t *step, int32_t set, void *stream);

/* ---- the pixel agent's choose_action (roborugby_amd/csrc/rr_cnn.hip; roborugby_amd/dqn.py PixelQNetwork / PixelDQNAgent): the forward of
 * the fixed convolutional Q network over n rows of planar uint8 pixels [n, channels, 64, 64] (PixelObservation(size=64, stack=1..4):
 * channels = 3 * stack), argmax and the epsilon-greedy draw, on the bf16 matrix cores.
 *   conv1 8x8, stride 4, no padding, ReLU: weight [16, channels, 8, 8], bias [16] -> [16, 15, 15]
 *   conv2 4x4, stride 2, no padding, ReLU: weight [32, 16, 4, 4],       bias [32] -> [32, 6, 6], flattened (c, y, x) to 1152
 *   fc1, ReLU: [256, 1152], [256];   fc2: [8, 256], [8] -> 8 Q-values
 * params = these eight tensors in that order (torch.nn layouts, fp32), read as they stand at call time: nothing is kept from one call
 * to the next (the first call allocates 635 KB of scratch in the handle, every call rewrites it; calls on one handle must be ordered,
 * e.g. on one stream).  The network's input is pixel * 2^-8 (not / 255).
 * THE ARITHMETIC (this is the specification; tests/cnn_ref.py is it in numpy):
 *   - in all four layers both operands of every product are bf16: a pixel's integer value 0..255 (exact in bf16), a weight rounded to
 *     nearest-even from the fp32 parameter, a hidden activation rounded to nearest-even after bias and ReLU;
 *   - the products are summed in fp32, in no particular order;
 *   - conv1's sum times 2^-8 (exact), every bias add and ReLU are fp32; the Q-values are the fp32 sums plus the fp32 bias.
 * actions[i] = the FIRST maximum of row i's Q-values, or with probability epsilon a uniform action: exactly rr_dqn_act's draw
 * (Philox4x32-10 of (seed, row, call), u <= epsilon, then word 1 & 7).  qvalues [n, 8] is optional (NULL: not written).
 * n: 1 .. 1<<22, any value (a last partial tile is masked: no row >= n is read or written).  pixels: contiguous, 16-byte aligned.
 * Returns -1 (message: rr_dqn_last_error) and launches nothing for a null handle / params entry / pixels / actions, channels outside
 * {3, 6, 9, 12}, n out of range, an epsilon that is NaN or outside [0, 1], a misaligned pixels.  Parameters must be finite. */
int rr_cnn_act(rr_dqn *dqn, const float *const params[8], const uint8_t *pixels, int32_t n, int32_t channels, float epsilon,
               uint64_t seed, uint32_t call, int32_t *actions, float *qvalues, void *stream);

/* ---- the SAC agent's choose_action (roborugby_amd/csrc/rr_sac.hip, rr_sac.hpp; roborugby_amd/sac.py ActorNetwork / BatchedSACAgent):
 * ActorNetwork.sample_normal (Training_SAC_pytorch.py:207-234) for n observations [n, 11] in one launch, on the fp32 matrix cores.
 * n_actions = A = 2 * nr_happy of the thrust entry (rr_step_thrust): 2 or 4.
 * params, in torch.nn.Linear layouts and fp32, read as they stand at call time (nothing is kept in the handle):
 *   fc1.weight [256,11], fc1.bias [256], fc2.weight [256,256], fc2.bias [256], mu.weight [A,256], mu.bias [A], sigma.weight [A,256],
 *   sigma.bias [A]
 * THE ARITHMETIC (this is the specification; tests/sac_ref.py is it in numpy):
 *   Forward.  ActorNetwork.forward (:192-205), fp32 throughout (rr_dqn_act's hidden layers: fp32 products summed in fp32, in no
 *     particular order): mu [A] and the raw sigma outputs [A]; sigma = clamp(raw, 1e-6, 1).
 *   Draw.  w0..w3 = Philox4x32-10 of counter (row, call, 0x5AC7, 0) under key (seed: low word, high word) -- rr_dqn_act's layout with
 *     another stream word, so one (seed, call) never correlates the two.  For the pair (w0, w1): u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1],
 *     u2 = (w1 >> 8) * 2^-24 in [0, 1), both exact in fp32; r = sqrtf(-2 logf(u1)), z0 = r cosf(2 pi u2), z1 = r sinf(2 pi u2).  The
 *     pair (w2, w3) gives z2 and z3 the same way.  A = 2 uses z0 and z1.  Pass a fresh `call` every time.
 *   Sample.  x_k = mu_k + sigma_k * z_k, actions[row][k] = max_action * tanhf(x_k),
 *     log_prob[row] = sum_k [ -z_k^2 / 2 - logf(sigma_k) - log(2 pi) / 2 - logf(1 - a_k^2 + 1e-6) ] with a_k the SCALED action, as the
 *     reference has it (:229-232).  With RR_SAC_DETERMINISTIC z = 0: actions = max_action * tanhf(mu), log_prob the formula at z = 0.
 * Outputs: actions [n, A] is required; log_prob [n], head [n, 2A] (mu[0..A), then the RAW sigma outputs before the clamp) and noise
 * [n, A] (the draws z; all 0 with RR_SAC_DETERMINISTIC) are each optional (NULL: not written).  Every element of every output that was
 * passed is written; no row >= n is read or written.
 * Returns -1 (message "rr_sac_act: ...": rr_dqn_last_error) and launches nothing for a null handle / params / params entry / obs /
 * actions, an n that is not a positive multiple of 64, n_actions outside {2, 4}, a max_action that is not finite and > 0, unknown flag
 * bits. */
#define RR_SAC_DETERMINISTIC 1      /* actions = max_action * tanh(mu); noise, if given, is written as 0 */
int rr_sac_act(rr_dqn *dqn, const float *const params[8], const float *obs, int32_t n, int32_t n_actions, float max_action,
               int32_t flags, uint64_t seed, uint32_t call, float *actions, float *log_prob, float *head, float *noise, void *stream);

/* ---- the no-grad half of the SAC agent's learn (roborugby_amd/csrc/rr_sac.hip k_sac_targets, rr_sac.hpp; roborugby_amd/sac.py
 * BatchedSACAgent.targets): the two vectors Agent.learn (Training_SAC_pytorch.py:344-383) computes without a gradient, for B replay rows
 * gathered out of the caller's rings, in ONE launch on the fp32 matrix cores:
 *   value_target[b] = min(Q1, Q2)(s_b, a~_b) - log pi(a~_b | s_b)      a~ a fresh (non-reparameterised) sample of the policy at s_b
 *   q_hat[b]        = reward_scale * r_b + gamma * (done_b ? 0 : V_target(s'_b))
 * The backward passes stay with the caller (autograd); `state` / `action` hand it the gathered rows it still needs.
 * Parameters in torch.nn.Linear layouts and fp32, read as they stand at call time (nothing is kept in the handle).
 * THE ARITHMETIC (this is the specification; tests/sac_targets_ref.py is it in numpy):
 *   Gather.  Batch row b takes ring row i = batch_index[b] (batch_index == NULL: i = b).  An i outside [0, mem_rows) is never used as an
 *     address: every output of that batch row that was passed is NaN (its `state` / `action` rows included); other batch rows are
 *     unaffected.
 *   Policy sample.  rr_sac_act's arithmetic on state_memory[i]: the head in fp32 (fp32 products summed in fp32, in no particular order),
 *     sigma = clamp(raw, 1e-6, 1), a~_k = max_action * tanhf(mu_k + sigma_k z_k), log_prob = rr_sac_act's formula with the SCALED action.
 *     noise == NULL: z = rr_sac_act's draw (Philox4x32-10, Box-Muller) of counter (b, call, 0x5A7A, 0) under key (seed: low word, high
 *     word) -- another stream word than rr_sac_act's 0x5AC7, so one (seed, call) never correlates acting and learning; the row word is the
 *     BATCH POSITION b, not the ring row.  noise != NULL: z = noise[b] ([B, A]).  Pass a fresh `call` every time.
 *   Critics.  q_j = CriticNetwork_j([s, a~]) (11 + A inputs; hidden layers as above), the single output an fp32 dot plus the fp32 bias.
 *     value_target = fminf(q1, q2) - log_prob: one subtraction of the two fp32 numbers the windows report.
 *   Next value.  v_next = ValueNetwork_target(new_state_memory[i]); the window reports it whether or not the row is terminal.
 *     q_hat = reward_scale * r + gamma * (done ? 0.0f : v_next), without contraction: fl(fl(reward_scale * r) + fl(gamma * v)), on a
 *     terminal row exactly fl(reward_scale * r).
 * Every element of every output that was passed is written for rows < B; nothing at or beyond row B is read or written; nothing is kept
 * in the handle; no atomics.  The results are bit-identical for any grid size (RR_DQN_WGS) and whether the draws came from the kernel or
 * were fed back through `noise` (noise_out of an earlier call).
 * Returns -1 (message "rr_sac_targets: ...": rr_dqn_last_error) and launches nothing for: a null handle, args or required pointer (a
 * parameter entry, a ring, value_target, q_hat), a wrong struct_size, a batch that is not a positive multiple of 64, n_actions outside
 * {2, 4}, mem_rows < 1, batch_index == NULL with mem_rows < batch, a max_action that is not finite and > 0, a non-finite gamma or
 * reward_scale, non-zero flags. */
typedef struct rr_sac_targets_args {
    int32_t struct_size;               /* = sizeof(rr_sac_targets_args) */
    int32_t batch;                     /* B: a positive multiple of 64 */
    int32_t n_actions;                 /* A: 2 or 4 */
    int32_t flags;                     /* 0 */
    const float *actor[8];             /* rr_sac_act's order */
    const float *critic_1[6], *critic_2[6];   /* fc1.weight [256, 11+A], fc1.bias, fc2.weight [256,256], fc2.bias, q.weight [1,256], q.bias [1] */
    const float *target_value[6];      /* fc1.weight [256,11], fc1.bias, fc2.weight, fc2.bias, v.weight [1,256], v.bias [1] */
    const float *state_memory, *new_state_memory;  /* [mem_rows, 11] */
    const float *action_memory;        /* [mem_rows, A] */
    const float *reward_memory;        /* [mem_rows] */
    const uint8_t *terminal_memory;    /* [mem_rows] (torch.bool) */
    int64_t mem_rows;                  /* rows of the rings that may be addressed: >= 1 */
    const int64_t *batch_index;        /* [B] rows of the rings; NULL: rows 0 .. B-1 (then mem_rows >= B) */
    const float *noise;                /* nullable [B, A]: the standard normal draws to use; NULL: the kernel draws */
    float max_action, gamma, reward_scale;
    uint64_t seed; uint32_t call;      /* key the draws when noise == NULL */
    float *value_target, *q_hat;       /* required, [B] each */
    float *state, *action;             /* nullable: the gathered rows [B,11], [B,A] (what the autograd half still needs) */
    float *policy_action, *log_prob, *head, *noise_out, *q1, *q2, *v_next;  /* nullable windows: [B,A], [B], [B,2A], [B,A], [B], [B], [B] */
} rr_sac_targets_args;
int rr_sac_targets(rr_dqn *dqn, const rr_sac_targets_args *args, void *stream);

/* ---- three of the four backward passes of the SAC agent's learn (roborugby_amd/csrc/rr_sac.hip k_sac_grads, k_sac_grads_reduce;
 * roborugby_amd/sac.py BatchedSACAgent.grads_fused): the gradients of the value loss and of the critic loss of Agent.learn
 * (Training_SAC_pytorch.py:344-383) with respect to the parameters of `value`, `critic_1` and `critic_2`, given the two target vectors
 * rr_sac_targets hands out, in one fused launch on the fp32 matrix cores plus one reduce launch -- no autograd:
 *   value_loss  = 0.5 * mse_loss(ValueNetwork(s), value_target)                                                     = loss[0]
 *   critic_loss = 0.5 * mse_loss(CriticNetwork_1([s, a]), q_hat) + 0.5 * mse_loss(CriticNetwork_2([s, a]), q_hat)   = loss[1] + loss[2]
 * The actor loss and its backward stay with the caller (autograd): it goes through both critics to the action and back through the
 * squashed policy.  No optimizer step is made here; the parameters are only read.
 * Inputs, all dense fp32: state [B,11], action [B,A], value_target [B], q_hat [B] (rr_sac_targets' outputs of those names, or any other
 * rows), and the six tensors of each net in rr_sac_targets_args' order and torch.nn.Linear layouts, read as they stand at call time.
 * Outputs: per net six gradient tensors in the same order and layouts, caller-owned, and loss [3].
 * THE ARITHMETIC (this is the specification; tests/sac_grads_ref.py is it in numpy float64):
 *   For net j with input x (value: s; critics: [s, a]) and target y (value: value_target; critics: q_hat), f = the fp32 forward:
 *     rr_sac_targets' hidden layers (fp32 products summed in fp32, in no particular order), then an fp32 dot plus the fp32 bias for the
 *     single output.  The output gradient of row b is d_b = (f_b - y_b) / B: one subtraction, one multiplication by fl(1 / B).
 *   loss[j] = 0.5 * mean_b (f_b - y_b)^2.
 *   The gradients are those of loss[j] by the chain rule through Linear -> ReLU -> Linear -> ReLU -> Linear; the ReLU derivative is
 *     h > 0 (0 at h == 0, as torch has it).  Every sum is fp32, in no particular order inside a 64-row tile; the tiles of a chunk are
 *     accumulated in order, the chunks summed in order.
 * Work split: with G workgroups (one per CU; RR_DQN_WGS bounds G) each net has C = max(1, G / 3) chunks, chunk c takes the 64-row tiles
 * c, c + C, ...; only the min(C, B / 64) chunks that have a tile enter the sum.
 * Every element of every output is written by every call; nothing at or beyond row B is read; no atomics; the handle keeps nothing but a
 * scratch for the per-chunk partial sums (allocated by the first call, grown by a call that needs more).  The results are bit-identical
 * from call to call for a given (B, G).  They are NOT promised identical across grid sizes (RR_DQN_WGS): the partial sums regroup.
 * One stream per handle at a time: the scratch is the handle's, so calls on two streams would share it; and the first call, or one that
 * needs more slots than any before, calls hipFree / hipMalloc -- make it outside a stream capture.
 * Inputs and parameters must be finite: a NaN row -- rr_sac_targets writes one for a ring row outside the rings -- makes the gradients
 * NaN; nothing here looks for it.
 * Returns -1 (message "rr_sac_grads: ...": rr_dqn_last_error) and launches nothing for: a null handle, args or required pointer (every
 * params and grads entry, state, action, value_target, q_hat, loss), a wrong struct_size, a batch that is not a positive
 * multiple of 64, n_actions outside {2, 4}, non-zero flags. */
typedef struct rr_sac_grads_args {
    int32_t struct_size;               /* = sizeof(rr_sac_grads_args) */
    int32_t batch;                     /* B: a positive multiple of 64 */
    int32_t n_actions;                 /* A: 2 or 4 */
    int32_t flags;                     /* 0 */
    const float *value[6];             /* fc1.weight [256,11], fc1.bias, fc2.weight [256,256], fc2.bias, v.weight [1,256], v.bias [1] */
    const float *critic_1[6], *critic_2[6];   /* fc1.weight [256, 11+A], fc1.bias, fc2.weight, fc2.bias, q.weight [1,256], q.bias [1] */
    const float *state, *action, *value_target, *q_hat;  /* [B,11], [B,A], [B], [B] */
    float *grad_value[6], *grad_critic_1[6], *grad_critic_2[6];  /* the gradients, in the parameters' order and layouts */
    float *loss;                       /* [3]: 0.5 * mse of value, critic_1, critic_2 */
} rr_sac_grads_args;
int rr_sac_grads(rr_dqn *dqn, const rr_sac_grads_args *args, void *stream);

/* ---- the frame-sharing pixel replay (roborugby_amd/csrc/rr_frames.hpp, rr_frames.hip; roborugby_amd/frame_replay.py FrameReplay): a ring
 * that stores every frame ONCE instead of two whole stacked observations per transition.  The caller owns the ring (device memory):
 *   frames  u8  [slots, rows, frame_bytes]   the newest frame of every row after push k, in slot k % slots
 *   age     u8  [slots, rows]                frames since the row's stack restarted: 0 where the row is `first` in this push (push 0:
 *                                            every row), otherwise min(age of push k - 1, plus 1, 255)
 *   action  i32 [slots, rows], reward f32 [slots, rows]
 *   flags   u8  [slots, rows]                bit 0: the step from push k - 1 to push k is a real transition of this row; bit 1: it ended
 *                                            the episode (terminal).  Push 0 writes 0.
 * `head` = the number of pushes so far, kept by the caller; push number k = head lands in slot head % slots.
 * The observation of row i at push k with stack S, oldest frame first: frame j (0 .. S-1) is the one of push k - min(S-1-j, age[k][i])
 * (PixelObservation's rule: a restarted row has every slot equal to its first frame).  Transition (k, i) = the stack at k - 1, action[k],
 * reward[k], terminal bit [k], the stack at k.  Sampleable: lo <= k <= head - 1 with lo = max(1, head - slots + S): every frame such a
 * transition needs is still in the ring.
 * Both entries take the rr_dqn handle for its device and the error string; they keep nothing in it.  Both return -1 (message:
 * rr_dqn_last_error) and launch nothing for: a null handle or required pointer, a partly-null metadata group, rows outside 1 .. 1<<22,
 * frame_bytes not a multiple of 16 in 16 .. 1 MiB, src_row_stride not a multiple of 16 in frame_bytes .. 1<<32, a src / frames / state /
 * next_state that is not 16-byte aligned, slots outside 2 .. 1<<31, head < 0.
 *
 * rr_frames_push: ONE launch copies row i's frame_bytes bytes from src + i * src_row_stride into slot head % slots (16-byte loads and
 * stores) and writes the row's four metadata words.  The newest frame of a stacked observation [rows, 3 * stack, 64, 64] is taken in place:
 * point src at its last three planes and pass the observation's row stride.  first [rows] (NULL: every row is first); action, reward,
 * done, valid: each [rows], all NULL (action 0, reward 0, flags 0: a push that only records frames) or all given; flags = (valid ? 1 : 0)
 * | (done ? 2 : 0).  Every byte of the slot's five arrays is written, nothing outside the slot; of the ring only `age` of slot
 * (head - 1) % slots is read. */
int rr_frames_push(rr_dqn *dqn, const uint8_t *src, int64_t src_row_stride, const uint8_t *first, const int32_t *action, const float *reward,
                   const uint8_t *done, const uint8_t *valid, int32_t rows, int64_t frame_bytes, int64_t slots, int64_t head,
                   uint8_t *frames, uint8_t *age, int32_t *action_ring, float *reward_ring, uint8_t *flags, void *stream);
/* rr_frames_sample: `batch` transitions out of the ring in one launch.  Per sample b:
 *   index == NULL (draw): attempts a = 0 .. 15 draw w = philox4x32_10(counter {b, call, 0x5A3E, a}, key = seed: low word, high word);
 *     k = lo + (((uint64)w[0] * (head - lo)) >> 32), row = ((uint64)w[1] * rows) >> 32.  The lowest a whose flags[k][row] has bit 0 set
 *     wins; none of the 16: ok[b] = 0.  Pass a fresh `call` every time.
 *   index [batch, 2] = (k, row): taken as it stands; a k outside the window, a row outside 0 .. rows-1 or a clear bit 0 give ok[b] = 0
 *     (such a value is never used as an index).
 *   ok[b] = 1: state / next_state [batch, stack, frame_bytes] = the two stacks as defined above, action, reward, terminal (0 / 1) of the
 *     transition, picked [batch, 2] (nullable) = (k, row).  ok[b] = 0: both stacks zero, action 0, reward 0, terminal 0, picked (-1, -1).
 * Every output element of rows 0 .. batch-1 is written, no row at or beyond batch is touched; at most stack + 1 frames are read per sample
 * for the 2 * stack it writes.  Also refused (-1): stack outside 1 .. 8, slots < stack + 1, batch outside 1 .. 1<<20, and in draw mode an
 * empty window (head - lo < 1). */
int rr_frames_sample(rr_dqn *dqn, const uint8_t *frames, const uint8_t *age, const int32_t *action_ring, const float *reward_ring,
                     const uint8_t *flags, int32_t rows, int64_t frame_bytes, int64_t slots, int64_t head, int32_t stack, int32_t batch,
                     const int64_t *index, uint64_t seed, uint32_t call, uint8_t *state, uint8_t *next_state, int32_t *action, float *reward,
                     uint8_t *terminal, uint8_t *ok, int64_t *picked, void *stream);

/* Introspection used by bench.py for the roofline line: bytes of the per-arena HBM record, and how many lanes of
 * a wavefront work on one arena (64 = one wavefront per arena; smaller = several arenas packed per wavefront). */
int rr_state_bytes_per_env(const rr_env *env, int64_t *bytes);
/* HBM copy probe for the roofline line: copies `bytes` (a multiple of 16, 16-byte aligned device buffers) from
 * src to dst with a 16-B-per-lane grid-stride kernel on the current device; the caller times it (HIP events) and quotes
 * 2 * bytes / time next to the 8 TB/s spec. */
int rr_probe_hbm_copy(void *dst, const void *src, size_t bytes, void *stream);
int rr_lanes_per_env(const rr_env *env, int32_t *lanes);

#ifdef __cplusplus
}
#endif
#endif /* ROBORUGBY_AMD_H */
