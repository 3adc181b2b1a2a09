/* tendon_hip.h -- C ABI of libtendon_hip.so: the MI355X (gfx950) batched tendon-robot
 * forward-kinematics + voxel-collision engine.
 *
 * This is the drop-in boundary for the reference's hot path (paths relative to the reference's
 * cpp/src/).  Plain pointers and sizes only.  Every entry point cites the reference interface it
 * stands in for; INTEGRATION.md shows the C++ shim (tendon::TendonRobot, collision::VoxelOctree,
 * motion_planning::VoxelBackboneValidityChecker / VoxelBackboneMotionValidator) a maintainer
 * adds on the reference side.
 *
 * Conventions
 *   - every function returns a tr_status (0 = ok); tr_last_error(ctx) gives the message.  The
 *     statuses map 1:1 to the C++ exception types the reference throws at the same conditions.
 *   - "states" are the reference's robot states: n x S row-major doubles,
 *     [tau_1..tau_N, (theta if enable_rotation), (s_start if enable_retraction)]
 *     (tendon/TendonRobot.h:105-115, motion-planning/AbstractValidityChecker.cpp:50-78).
 *   - *_dev entry points take DEVICE pointers and a hipStream_t (as void*); they enqueue work and
 *     return without synchronising.  The host-pointer forms copy in/out and synchronise.
 *   - one context = one workspace (fallback list, point columns, ordering buffers, argument slots are
 *     per context).  Entry points serialise on a per-context mutex, and the *_dev calls that touch that
 *     workspace execute in ISSUE ORDER whichever streams they name: a call arriving on a different
 *     stream than the previous one first makes its stream wait (hipStreamWaitEvent) for that call's
 *     work.  So two caller streams never share the scratch concurrently, and there is no concurrency
 *     to gain from several streams on ONE context -- use one context per concurrent stream
 *     (contexts share nothing but the device).  Caller buffers are the caller's to order.
 *   - validity bitmasks: bit (i & 63) of word (i >> 6) is configuration i; padding bits are 0.
 *   - non-convergence / NaN in a lane is not an error: that configuration is simply invalid.
 */
#ifndef TENDON_HIP_H
#define TENDON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TR_MAX_TENDONS 8
#define TR_MAX_COEF    8

typedef enum {
  TR_OK                = 0,
  TR_ERR_INVALID_ARG   = 1,  /* std::invalid_argument: state size, dims, dL vs voxel size ...   */
  TR_ERR_OUT_OF_RANGE  = 2,  /* std::out_of_range: tendon / tau count mismatch                  */
  TR_ERR_DOMAIN        = 3,  /* std::domain_error: point outside the voxel domain (find_cell)   */
  TR_ERR_LENGTH        = 4,  /* std::length_error: non-positive voxel limits                    */
  TR_ERR_RUNTIME       = 5,  /* std::runtime_error                                              */
  TR_ERR_HIP           = 6,  /* HIP runtime failure (message carries hipGetErrorString)          */
  TR_ERR_UNSUPPORTED   = 7   /* feature of the reference not offered by this build              */
} tr_status;

/* tendon::TendonRobot + BackboneSpecs + TendonSpecs (tendon/TendonRobot.h:52-58,
 * tendon/BackboneSpecs.h:14-20, tendon/TendonSpecs.h:25-30).  All tendons share n_a = C.size()
 * and n_m = D.size(), as get_r_info assumes (tendon/get_r_info.cpp:112-115). */
typedef struct {
  double  r;                       /* robot radius (m)                                         */
  double  L, dL, ro, ri, E, nu;    /* backbone                                                  */
  int32_t n_tendons, n_a, n_m;
  const double *C;                 /* n_tendons x n_a row-major: theta_i(t) = sum C[i][k] t^k   */
  const double *D;                 /* n_tendons x n_m row-major: rho_i(t)   = sum D[i][k] t^k   */
  const double *max_tension;       /* [n_tendons]                                               */
  const double *min_length;        /* [n_tendons]                                               */
  const double *max_length;        /* [n_tendons]                                               */
  int32_t enable_rotation, enable_retraction;
  double  residual_threshold;
} tr_robot_desc;

typedef struct tr_ctx tr_ctx;

/* flag bits written per configuration by the validate calls (optional output) */
#define TR_FLAG_CONVERGED   1u   /* fk.converged && home.converged                               */
#define TR_FLAG_LENGTH_OK   2u   /* is_within_length_limits                                      */
#define TR_FLAG_NO_SELFCOL  4u   /* !collides_self                                               */
#define TR_FLAG_NO_VOXCOL   8u   /* !collides(voxelize(fk))                                      */
#define TR_FLAG_DOMAIN     16u   /* a backbone point was non-finite or absurdly far outside the
                                    voxel domain (reference: undefined behaviour); forced invalid */

/* ---- life cycle ------------------------------------------------------------------------- */

/* Replaces constructing a tendon::TendonRobot (TendonRobot::from_toml, tendon/TendonRobot.cpp:1033-1089)
 * plus the per-call constants of tension_shape (get_stiffness_matrices, t_range,
 * tendon/TendonRobot.cpp:69-84,105-148).  device = HIP device ordinal. */
int tr_create(const tr_robot_desc *robot, int device, tr_ctx **out);
void tr_destroy(tr_ctx *ctx);
const char *tr_last_error(const tr_ctx *ctx);   /* ctx may be NULL: last create error */

int tr_state_size(const tr_ctx *ctx);           /* TendonRobot::state_size, TendonRobot.h:60-64 */
int tr_num_points(const tr_ctx *ctx);           /* |t_range(0, L, dL)| = max backbone points    */
int tr_device(const tr_ctx *ctx);

/* Opens (on != 0) or closes the context to LOADED shapes of a robot with retraction.  A context never opened refuses such a robot in
 * every loaded call with one message, TR_ERR_UNSUPPORTED, as it always did.  Opened: tr_fk_loaded_batch*, tr_fk_loaded_tips* (and with
 * them general_shape and the validity of loaded shapes) take the robot, see tr_fk_loaded_batch; the loaded calls built on them --
 * edges, roadmap builds, IK, Jacobian and compliance, tip queries, load profiles -- keep answering TR_ERR_UNSUPPORTED, now each under
 * its own name.  No effect on a robot without retraction.
 * on == TR_LOADED_RETRACTION_EDGES (2) opens what 1 opens plus the loaded edge checks (tr_validate_edges_loaded with and without
 * last_valid_t, tr_validate_edges_loaded_indexed and its pairwise fall-back, tr_edges_loaded_vertex_strains, tr_edges_loaded_last; see
 * tr_validate_edges_loaded for what a sample of such a robot is).  The voxel forms of the loaded edges, the loaded roadmap builds, IK,
 * Jacobian and compliance, tip queries and load profiles refuse at this level too.  Any other non-zero value means 1.
 * tr_loaded_retraction returns the level (-1: ctx == NULL). */
enum { TR_LOADED_RETRACTION_OFF = 0, TR_LOADED_RETRACTION_FK = 1, TR_LOADED_RETRACTION_EDGES = 2 };
int tr_set_loaded_retraction(tr_ctx *ctx, int on);
int tr_loaded_retraction(const tr_ctx *ctx);
/* A robot with retraction: a wave of the loaded FK runs from its longest backbone's base to the tip while its shorter lanes idle, so a
 * call of at least TENDON_HIP_LOADED_RETRACT_SORT problems (read at tr_create; 0: never) is solved in the order of its problems'
 * s_start -- inside the call: every input row is read and every output row written at the caller's index, and the results are the
 * bits of the arrival-order solve.  This holds for every caller of the shooting: tr_fk_loaded_batch*, tr_fk_loaded_tips* (per chunk),
 * the validity of loaded shapes, every level of the loaded edge calls and the indexed form's vertex block.
 * stats = problems of the context's last shooting run (one such call, chunk or level), how many of them were solved in order. */
int tr_loaded_order_last(const tr_ctx *ctx, int64_t stats[2]);

/* Home shape tendon lengths at s_start = 0 (TendonRobot::home_shape, tendon/TendonRobot.cpp:249-314) */
int tr_home_lengths(const tr_ctx *ctx, double *L_i /*[n_tendons]*/);

/* Replaces the VoxelOctree obstacle member + VoxelEnvironment rotation held by the voxel
 * validity checkers (motion-planning/AbstractVoxelValidityChecker.h:63-64,
 * VoxelEnvironment.cpp:129-131).  blocks: HOST pointer, Nb^3 uint64 (Nb = N/4), index
 * ((bx*Nb)+by)*Nb+bz, bit x*16+y*4+z inside a block (collision/VoxelOctree.cpp:1501-1503).
 * lim = {xmin,xmax,ymin,ymax,zmin,zmax}.  inv_rot: row-major 3x3 (NULL = identity).
 * Fails with TR_ERR_INVALID_ARG when dL > max voxel edge, as VoxelBackboneValidityChecker's
 * constructor does (motion-planning/VoxelBackboneValidityChecker.h:37-45). */
int tr_set_grid(tr_ctx *ctx, uint32_t N, const double lim[6], const uint64_t *blocks,
                const double inv_rot[9]);

/* Which state validity checker is installed (si->setStateValidityChecker, motion-planning/Problem.h:175-197):
 * TR_CHECKER_BACKBONE = motion_planning::VoxelBackboneValidityChecker (the backbone polyline against a
 * pre-dilated environment, VoxelBackboneValidityChecker.h:28-58; the default),
 * TR_CHECKER_SPHERES  = motion_planning::VoxelValidityChecker (a sphere of the robot radius at every
 * backbone point against the raw environment, VoxelValidityChecker.h:18-26).
 * It decides tr_validate_batch* (isValid) and -- exactly where the reference's motion validators ask the installed
 * checker, `_vc->collides(shape)` in voxelize_until_invalid_impl (VoxelBackboneMotionValidator.cpp:83-91) -- the
 * per-sample test of the checkMotion(s1, s2, last_valid) forms: tr_validate_edges_last_valid and
 * tr_validate_edges_discrete with a last_valid_t output.  checkMotion(s1, s2) itself (tr_validate_edges,
 * tr_validate_edges_indexed, tr_validate_edges_discrete without last_valid_t) and the voxel caches (tr_voxelize_*)
 * sweep the BACKBONE against the voxels under either checker, as AbstractVoxelMotionValidator::checkMotion does
 * (AbstractVoxelMotionValidator.h:143-151: voxelize() = is_valid_shape only, then collides(partial.voxels)).
 * Call it before tr_set_grid: the dL <= voxel size check of tr_set_grid is the backbone checker's constructor check
 * and is skipped for TR_CHECKER_SPHERES. */
#define TR_CHECKER_BACKBONE 0
#define TR_CHECKER_SPHERES 1
int tr_set_checker(tr_ctx *ctx, int32_t checker);

/* ---- environment preparation on the resident obstacle grid ------------------------------
 * collision::VoxelOctree's editing operations, applied to the grid tr_set_grid uploaded, without it
 * leaving the device (apps/prepare_voxel_env.cpp:247-315 runs them on the host octree):
 *   tr_grid_add_spheres      add_sphere for n spheres, (cx, cy, cz, r) each (VoxelOctree.cpp:434-469)
 *   tr_grid_add_capsules     add_capsule for n capsules, (ax, ay, az, bx, by, bz, r) each (:471-515) -- with add_spheres
 *                            everything Environment::voxelize rasterises (motion-planning/Environment.cpp:62-100)
 *   tr_grid_remove_interior  remove_interior(keep_diagonal) (:533-689; VoxelOctree.h:207-210)
 *   tr_grid_dilate           dilate(num, use_diagonal) (:693-818; VoxelOctree.h:215-218)
 *   tr_grid_dilate_sphere    dilate_sphere(r) (:950-952)
 *   tr_get_grid              download the current blocks ((N/4)^3 words, layout as tr_set_grid) */
int tr_grid_add_spheres(tr_ctx *ctx, const double *spheres, int64_t n);
int tr_grid_add_capsules(tr_ctx *ctx, const double *capsules, int64_t n);
int tr_grid_remove_interior(tr_ctx *ctx, int32_t keep_diagonal);
int tr_grid_dilate(tr_ctx *ctx, int32_t num, int32_t use_diagonal);
int tr_grid_dilate_sphere(tr_ctx *ctx, double r);
int tr_get_grid(tr_ctx *ctx, uint64_t *blocks);

/* Pre-size the device workspace for batches of up to n configurations (optional; the batch
 * calls grow it on demand, which allocates and therefore synchronises). */
int tr_reserve(tr_ctx *ctx, int64_t n);

/* Pre-size the FK sample pool and the device frontier of the edge calls (tr_validate_edges*,
 * tr_voxelize_edges) for batches of up to n_edges edges (optional, as above). */
int tr_reserve_edges(tr_ctx *ctx, int64_t n_edges);

/* ---- forward kinematics: TendonRobot::shape / forward_kinematics ------------------------ */

/* Batched TendonRobot::shape(state) (tendon/TendonRobot.h:105-131 -> tension_shape,
 * tendon/TendonRobot.cpp:325-500), replacing the omp-parallel loops at
 * apps/estimate_length_discretization.cpp:62-71 and apps/roadmap2samples.cpp:65-78.
 * Host buffers; any output pointer may be NULL.
 *   p         n x P x 3   backbone points (rows past n_points[i] are NaN), P = tr_num_points
 *   R         n x P x 9   rotation matrices, column-major per matrix (Eigen layout)
 *   L, L_i    n, n x N    backbone / tendon lengths
 *   converged n           TendonResult::converged
 *   n_points  n           points of configuration i (P unless retraction shortens it)      */
int tr_fk_batch(tr_ctx *ctx, const double *states, int64_t n,
                double *p, double *R, double *L, double *L_i, uint8_t *converged, int32_t *n_points);

/* Device form.  Points are written structure-of-arrays, lane-contiguous:
 * d_px[j*ld + i] is x of point j of configuration i (ld >= n, multiple of 64).  d_R (optional)
 * is [9][P][ld].  d_Li is [N][ld].
 * With retraction enabled a configuration has d_n_points[i] <= P points and its rows are aligned at the
 * TIP: point j of configuration i is in row j + (P - d_n_points[i]) (the tip always in row P - 1). */
int tr_fk_batch_dev(tr_ctx *ctx, const double *d_states, int64_t n, int64_t ld,
                    double *d_px, double *d_py, double *d_pz, double *d_R,
                    double *d_L, double *d_Li, uint8_t *d_converged, int32_t *d_n_points,
                    void *stream);

/* The same for retraction-enabled robots, whose home-shape tendon lengths depend on the configuration
 * (home_shape(s_start), tendon/TendonRobot.cpp:249-314): d_n_points and d_home_Li ([N][ld]) are mandatory
 * outputs; rows are aligned at the tip as described above.  Feeds tr_validate_shapes_retraction_dev. */
int tr_fk_batch_retraction_dev(tr_ctx *ctx, const double *d_states, int64_t n, int64_t ld,
                               double *d_px, double *d_py, double *d_pz, double *d_R,
                               double *d_L, double *d_Li, uint8_t *d_converged, int32_t *d_n_points,
                               double *d_home_Li, void *stream);

/* ---- tip positions, tip Jacobian, tip IK: tip_control::inverse_kinematics ------------------- */

/* fk_shape(state).p.back() for n states (tip_control.cpp:96-104 before its retraction wrapper):
 * tips n x 3, converged (optional) n.  One K1 launch with only the tips stored: the same instantiation
 * tr_fk_batch runs, so the tips are the bits of tr_fk_batch's last point. */
int tr_fk_tips(tr_ctx *ctx, const double *states, int64_t n, double *tips, uint8_t *converged);
int tr_fk_tips_dev(tr_ctx *ctx, const double *d_states, int64_t n, double *d_tips, uint8_t *d_converged, void *stream);

/* The central-difference tip Jacobian levmar forms inside tip_control::inverse_kinematics
 * (tip_control.cpp:35-140 with opts[4] = -finite_difference_delta; 3rdparty/levmar-2.6/misc_core.c:175-211),
 * through tip_control's FK wrapper (a retraction beyond L has its tip at (0, 0, L - s_start),
 * tip_control.cpp:96-104): per column j, d_j = max(|1e-4 p_j|, delta),
 * J[:, j] = (tip(p + d_j e_j) - tip(p - d_j e_j)) * (0.5 / d_j).  All n (2 S + 1) FK evaluations of a call are
 * one K1 launch (chunked internally).  J: n x 3 x S row-major; tips (optional): n x 3, f(p) through the wrapper. */
int tr_tip_jacobian(tr_ctx *ctx, const double *states, int64_t n, double delta, double *tips, double *J);
int tr_tip_jacobian_dev(tr_ctx *ctx, const double *d_states, int64_t n, double delta, double *d_tips, double *d_J, void *stream);

/* The arguments of tip_control::inverse_kinematics after the start and the goal (tip_control.h:88-100);
 * a NULL tr_ik_params* means the defaults written there: 100, 0.1, 1e-9, 1e-4, 1e-4, 1e-6. */
typedef struct {
  int32_t max_iters;
  double  mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, stop_threshold_err, finite_difference_delta;
} tr_ik_params;

/* Batched tip_control::inverse_kinematics (tip_control.cpp:35-140), one start state per problem, n problems at once
 * (VoxelCachedLazyPRM::roadmapIk runs k of them, motion-planning/VoxelCachedLazyPRM.cpp:3164-3205).  The optimiser is this
 * library's own projected Levenberg-Marquardt with levmar's central-difference Jacobian, gain-ratio damping and the same four stop
 * tests (it is not levmar's code path); every problem's state stays on the device, and one round -- one K1 launch of the
 * 2 S + 1 evaluations of every still-active problem plus one LM-step launch -- advances all of them by an iteration.
 *   initial_states  n x S (clipped to the bounds first)
 *   des             n x 3 goal tips with row stride des_ld doubles, or one goal for all when des_ld == 0
 *   lo, hi          S each; NULL = Bounds::from_robot (tip_control.cpp:160-185)
 *   states_out      n x S solved states, rotation canonical in [-pi, pi) (util/angles.h:13-34)
 *   tips_out, error_out, iters_out, fk_calls_out   IKResult::tip, error, iters, num_fk_calls (a multiple of 2 S + 1)
 *   rounds_out      rounds run (a host pointer in both forms)
 * Every output may be NULL.  A problem's result does not depend on the other problems of the call or on their order. */
int tr_ik_batch(tr_ctx *ctx, const tr_ik_params *params, const double *initial_states, int64_t n, const double *des, int64_t des_ld,
                const double *lo, const double *hi, double *states_out, double *tips_out, double *error_out,
                int32_t *iters_out, int32_t *fk_calls_out, int64_t *rounds_out);
/* Device form: device arrays, host lo / hi / params / rounds_out.  It synchronises `stream` once per round to read the number of
 * problems still active (4 bytes through pinned memory); nothing else crosses the bus. */
int tr_ik_batch_dev(tr_ctx *ctx, const tr_ik_params *params, const double *d_initial_states, int64_t n, const double *d_des,
                    int64_t des_ld, const double *lo, const double *hi, double *d_states_out, double *d_tips_out,
                    double *d_error_out, int32_t *d_iters_out, int32_t *d_fk_calls_out, int64_t *rounds_out, void *stream);

/* ---- loaded forward kinematics: TendonRobot::general_shape --------------------------------- */

/* The arguments of TendonRobot::general_shape after the loads and the guess (tendon/TendonRobot.h:199-203); a NULL
 * tr_shoot_params* means the defaults written there: 100, 0.1, 1e-9, 1e-4, 1e-6. */
typedef struct {
  int32_t max_iters;
  double  mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, finite_difference_delta;
} tr_shoot_params;

/* Batched TendonRobot::general_shape (tendon/TendonRobot.h:155-219 -> general_tension_shape, tendon/TendonRobot.cpp:689-952):
 * the shape of the rod under a tip force and moment F_e, L_e and a distributed force and moment f_e, l_e per unit length, all
 * in the robot's base frame BEFORE the state's rotation (general_shape rotates the solved shape).  It is a boundary-value
 * problem: classical RK4 over t_range(0, L, dL) from p = 0, R = I and base strains (v0, u0) with tendon_deriv's loaded right-hand
 * side (tendon_deriv.cpp:331-332), solved for the six strains by single shooting until the tip balance
 * e = (F_e_est - F_e, L_e_est - L_e) of PointForces::calc_point_forces (TendonRobot.cpp:188-217, routing at s = L) vanishes.
 *   - The distributed load is ONE CONSTANT VECTOR PAIR per problem (gravity), times the context's load profile w(s) where one is
 *     installed (tr_set_load_profile, below).  The reference takes functions of (t, p); a load whose direction varies along the
 *     backbone, and a position-dependent load, are not offered.
 *   - The optimiser is this library's own Levenberg-Marquardt (tr_ik_batch's, without bounds) with levmar's central-difference
 *     Jacobian (d_j = max(|1e-4 p_j|, delta)) and gain-ratio damping; it is not levmar's code path.  The damping term is
 *     mu diag(J^T J) with mu starting at mu_init (Marquardt's scaling: strains, curvatures, forces and moments put nine decades
 *     into diag(J^T J), and mu_init max diag(J^T J) times the identity freezes the bending directions), and the step that the
 *     |Dp| test judges small is still evaluated before the problem ends.  Stops: |e| <=
 *     residual_threshold -> converged (levmar's reason 6, the only one general_tension_shape reports as converged);
 *     |J^T e|_inf <= stop_threshold_JT_err_inf; |Dp| <= stop_threshold_Dp |p|; max_iters; a non-finite residual.  All but the first
 *     report not converged; none is an error of the call.
 *   - Start: guess (n x 6 rows (v, u)), or with guess == NULL the UNLOADED solution of the problem's tensions
 *     (solve_initial_bending), not the reference's straight rod (v, u) = (e3, 0).  At zero load that start already balances the
 *     tip, so the call takes zero iterations and returns tr_fk_batch's shape; under load it is a few iterations from the answer.
 *   - All 13 integrations of an iteration (the trial point and its 12 neighbours) of all still-active problems are one launch;
 *     one round = expansion, integration, LM step.  Problems are solved in chunks that bound the workspace.
 *   states    n x S                 wrench   (F_e, L_e) rows with stride wrench_ld >= 6, or one row for all (wrench_ld == 0);
 *                                            NULL = no tip wrench
 *   dist      (f_e, l_e) rows with stride dist_ld >= 6, one row for all (dist_ld == 0), NULL = none
 *   p, R, L, L_i, n_points          tr_fk_batch's outputs, of the integration at the final strains
 *   converged n                     |e| <= residual_threshold at the final strains
 *   vu0_out   n x 6 final (v0, u0); vuL_out n x 6: the strains (v, u) at the tip (TendonResult::v_f, u_f);
 *   residual_out n: |e| at the final strains; iters_out n: LM steps taken;
 *   fk_calls_out n: integrations of the solve (1 for the start, 13 per round after it; the launch that writes the outputs
 *   is not counted); rounds_out: rounds run, a host pointer in both forms.
 * Every output may be NULL.  A problem's result does not depend on the other problems of the call, their order or the chunking.
 * Robots with retraction: TR_ERR_UNSUPPORTED unless the context was opened to them (tr_set_loaded_retraction).  Then
 * (general_tension_shape's s_start, TendonRobot.cpp:689-952, read from the state as general_shape reads it,
 * TendonRobot.h:177-208): a problem shoots on t_range(s_start, L, dL) from the unloaded solution AT its s_start; it has
 * n_points[i] <= P points, p and R start at row 0 and are NaN in the rows past n_points[i], as tr_fk_batch's.  s_start >= L (it is
 * truncated to L): one point at the origin, L = L_i = 0, n_points = 1, converged = 1 after zero iterations (the reference's early
 * return); s_start < 0: the same with converged = 0, as tr_fk_batch reports it.  The loaded calls built on this one -- edges, roadmap
 * builds, IK, Jacobian and compliance, tip queries, load profiles -- answer TR_ERR_UNSUPPORTED on such a robot, each under its own
 * name; on a context that was never opened every loaded call answers with the one message it always had. */
int tr_fk_loaded_batch(tr_ctx *ctx, const tr_shoot_params *params, const double *states, int64_t n,
                       const double *wrench, int64_t wrench_ld, const double *dist, int64_t dist_ld, const double *guess,
                       double *p, double *R, double *L, double *L_i, uint8_t *converged, int32_t *n_points,
                       double *vu0_out, double *vuL_out, double *residual_out, int32_t *iters_out, int32_t *fk_calls_out,
                       int64_t *rounds_out);
/* Device form: device arrays in tr_fk_batch_dev's layout (d_px[j*ld + i], d_R [9][P][ld], d_Li [N][ld]; ld >= n, a multiple of 64),
 * host params / rounds_out.  d_px, d_py, d_pz, d_Li, d_converged feed tr_validate_shapes_dev unchanged.  It synchronises `stream`
 * once per round to read the number of problems still active (4 bytes through pinned memory).
 * With retraction enabled a configuration has d_n_points[i] <= P points and its rows are aligned at the tip, as tr_fk_batch_dev
 * describes: point j is in row j + (P - d_n_points[i]) of the planes and of d_R; the rows before it are not written. */
int tr_fk_loaded_batch_dev(tr_ctx *ctx, const tr_shoot_params *params, const double *d_states, int64_t n, int64_t ld,
                           const double *d_wrench, int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess,
                           double *d_px, double *d_py, double *d_pz, double *d_R, double *d_L, double *d_Li, uint8_t *d_converged,
                           int32_t *d_n_points, double *d_vu0_out, double *d_vuL_out, double *d_residual_out, int32_t *d_iters_out,
                           int32_t *d_fk_calls_out, int64_t *rounds_out, void *stream);

/* The same for retraction-enabled robots, whose home-shape tendon lengths depend on the configuration (home_shape(s_start).L_i,
 * d_home_Li [N][ld]): the loaded twin of tr_fk_batch_retraction_dev.  d_n_points and d_home_Li are mandatory outputs; d_px, d_py,
 * d_pz, d_n_points, d_Li, d_home_Li and d_converged feed tr_validate_shapes_retraction_dev unchanged.  The call's name says what it
 * is for: it needs no tr_set_loaded_retraction.  A robot without retraction: TR_ERR_INVALID_ARG. */
int tr_fk_loaded_batch_retraction_dev(tr_ctx *ctx, const tr_shoot_params *params, const double *d_states, int64_t n, int64_t ld,
                                      const double *d_wrench, int64_t wrench_ld, const double *d_dist, int64_t dist_ld,
                                      const double *d_guess, double *d_px, double *d_py, double *d_pz, double *d_R, double *d_L,
                                      double *d_Li, uint8_t *d_converged, int32_t *d_n_points, double *d_home_Li, double *d_vu0_out,
                                      double *d_vuL_out, double *d_residual_out, int32_t *d_iters_out, int32_t *d_fk_calls_out,
                                      int64_t *rounds_out, void *stream);

/* A load profile: a scalar weight w(s) along arc length that every loaded call of the context applies to its distributed load.  At
 * every RK4 stage a problem sees w(s) f_e, w(s) l_e, where (f_e, l_e) is the row the call would use without a profile (per-problem
 * rows in tr_fk_loaded_batch, the call's one set after its frame handling elsewhere); the tip wrench is not scaled.  This is
 * f_e(t) = rho(t) g: a mass that varies along the backbone, under gravity.  A load whose DIRECTION varies with s, or any dependence
 * on the position p, is not offered.
 *   w is piecewise linear over n_knots >= 1 knots (s[k], w[k]): s strictly increasing and finite, w finite; outside
 *   [s[0], s[n_knots - 1]] the end value holds; for x in [s[k], s[k+1]]  w = w[k] + (w[k+1] - w[k]) * ((x - s[k]) / (s[k+1] - s[k]))
 *   in this operation order, in fp64, without contraction, with k the LAST knot at or below x (so a knot's own weight holds at
 *   the knot exactly).
 * The host evaluates w once into a table of 1 + 3 n_steps doubles at the abscissae of the RK4 stages, indexed like the routing
 * table: entry 0 at s = 0; entries 1 + 3k, 1 + 3k + 1, 1 + 3k + 2 at t_k, t_k + h_k * 0.5, t_k + h_k of step k.  The kernels read a
 * stage's weight from it and form w * f_e[q], w * l_e[q], each product rounded once.
 * tr_set_load_profile first waits for the context's device work (a queued *_dev call keeps the profile it was issued under), then
 * installs the table; tr_clear_load_profile removes it (the calls run as without one).  Robots with retraction:
 * TR_ERR_UNSUPPORTED (the table has no entries for a configuration's own first interval).  Bad knots or weights:
 * TR_ERR_INVALID_ARG. */
int tr_set_load_profile(tr_ctx *ctx, int64_t n_knots, const double *s, const double *w);
int tr_clear_load_profile(tr_ctx *ctx);
/* The installed table: *n_out = its length (0: no profile installed); table_out (may be NULL) receives min(capacity, *n_out) entries. */
int tr_get_load_profile(tr_ctx *ctx, double *table_out, int64_t capacity, int64_t *n_out);

/* ---- state validity: StateValidityChecker::isValid -------------------------------------- */

/* Batched AbstractValidityChecker::isValid (motion-planning/AbstractValidityChecker.cpp:124-133)
 * with VoxelBackboneValidityChecker::voxelize_impl + collides
 * (VoxelBackboneValidityChecker.h:49-57, AbstractVoxelValidityChecker.h:55-57): FK, converged,
 * tendon-length limits, self-collision, backbone voxelisation vs the obstacle grid.  Replaces the
 * loops at motion-planning/VoxelCachedLazyPRM.cpp:1448-1455 and :1584-1591.
 *   valid_bits  ceil(n/64) words
 *   tips        n x 3 (optional)  fk_shape.p.back() (VoxelCachedLazyPRM.cpp:1438)
 *   flags       n (optional)      TR_FLAG_* bits                                            */
int tr_validate_batch(tr_ctx *ctx, const double *states, int64_t n,
                      uint64_t *valid_bits, double *tips, uint8_t *flags);
int tr_validate_batch_dev(tr_ctx *ctx, const double *d_states, int64_t n,
                          uint64_t *d_valid_bits, double *d_tips, uint8_t *d_flags, void *stream);

/* ---- createRoadmap phase 1 on the device: rejection sampling of valid vertices ------------- */

/* The reference's vertex phase (motion-planning/VoxelCachedLazyPRM.cpp:1415-1455) draws every new milestone in a loop
 *   sampleUniform -> fk -> is_valid_shape -> voxelize -> collides   until a state is accepted (:1441-1444),
 * from thread-local OMPL generators (not reproducible).  Here the candidates form ONE sequence that is a pure function of
 * (seed, candidate index): Philox-4x32-10 with counter (index, coordinate pair) and key = seed gives 53-bit uniforms u,
 * state[d] = lo[d] + u * (hi[d] - lo[d]) (product and sum rounded separately).  lo / hi: S doubles each, or both NULL for the
 * planner's state-space bounds (Problem.cpp:101-163: tension [0, max_tension_i], rotation [-pi, pi), retraction [0, L]).
 * The same candidates come out for every batch size, every GPU count (rank g takes a contiguous index range) and from the
 * host mirror (interactive-rate-tendons_amd/distributed.py: candidate_states).  States are generated in HBM and never
 * uploaded. */
int tr_candidate_states(tr_ctx *ctx, uint64_t seed, uint64_t first, int64_t count, const double *lo, const double *hi,
                        double *states /* count x S, host */);
int tr_candidate_states_dev(tr_ctx *ctx, uint64_t seed, uint64_t first, int64_t count, const double *lo, const double *hi,
                            double *d_states /* count x S */, void *stream);

/* tr_validate_batch_dev on candidates [first, first + count) of the sequence, generated on the device (first % 64 == 0 so
 * that shards are whole mask words).  The shard form of config 4: the mask stays on the device for the all-gather. */
int tr_validate_candidates_dev(tr_ctx *ctx, uint64_t seed, uint64_t first, int64_t count, const double *lo, const double *hi,
                               uint64_t *d_valid_bits, double *d_tips, uint8_t *d_flags, void *stream);

/* Order-preserving compaction on the device: rows i of d_rows (row_doubles doubles each) whose mask bit is set go, in
 * ascending i, to d_rows_out (at most `capacity` rows); d_index_out (optional) receives their i.  *n_out = number of set
 * bits among the first `count` (rows written = min(*n_out, capacity)).  With the gathered vertex mask and the regenerated
 * candidates this yields the same vertex array on every rank.  Synchronises `stream` (one counter read-back). */
int tr_compact_rows_dev(tr_ctx *ctx, const uint64_t *d_mask, int64_t count, const double *d_rows, int32_t row_doubles,
                        int64_t capacity, double *d_rows_out, int64_t *d_index_out, int64_t *n_out, void *stream);

/* The whole loop: candidates first_candidate, first_candidate + 1, ... are validated batch by batch (fk_verdict; batch sizes
 * follow the acceptance rate seen so far) and the first n_want VALID ones are returned in candidate order -- the accepted set
 * does not depend on the batch sizes.  One 32-byte counter read-back per batch is the only host traffic of the _dev form.
 *   states  n_want x S     tips  n_want x 3 (optional)     index  n_want (optional): candidate index of each vertex
 *   *n_accepted  vertices returned (< n_want only when max_candidates candidates did not yield enough; 0 = the default
 *                64 n_want + 2^20)        *n_tried  candidates consumed up to and including the last accepted one         */
int tr_sample_valid_vertices(tr_ctx *ctx, uint64_t seed, uint64_t first_candidate, const double *lo, const double *hi,
                             int64_t n_want, int64_t max_candidates, double *states, double *tips, int64_t *index,
                             int64_t *n_accepted, int64_t *n_tried);
int tr_sample_valid_vertices_dev(tr_ctx *ctx, uint64_t seed, uint64_t first_candidate, const double *lo, const double *hi,
                                 int64_t n_want, int64_t max_candidates, double *d_states, double *d_tips, int64_t *d_index,
                                 int64_t *n_accepted, int64_t *n_tried, void *stream);

/* The second stage alone, on caller-supplied backbone shapes (is_valid_shape + voxelize +
 * collides on given TendonResults: AbstractValidityChecker.cpp:99-122).  Device pointers, SoA as
 * produced by tr_fk_batch_dev.  d_n_points is ignored (a robot without retraction has all P points in
 * every configuration; kept in the signature for symmetry).  check_voxels = 0 skips the
 * obstacle test (the "is_valid_shape only" predicate used while voxelising edges,
 * VoxelBackboneMotionValidator.cpp:29-36).  Retraction-enabled robots: the _retraction_ form below. */
int tr_validate_shapes_dev(tr_ctx *ctx, int64_t n, int64_t ld,
                           const double *d_px, const double *d_py, const double *d_pz,
                           const int32_t *d_n_points, const double *d_Li, const uint8_t *d_converged,
                           int check_voxels, uint64_t *d_valid_bits, uint8_t *d_flags, void *stream);
/* ... on the outputs of tr_fk_batch_retraction_dev (per-configuration point counts and home lengths). */
int tr_validate_shapes_retraction_dev(tr_ctx *ctx, int64_t n, int64_t ld,
                                      const double *d_px, const double *d_py, const double *d_pz,
                                      const int32_t *d_n_points, const double *d_Li, const double *d_home_Li,
                                      const uint8_t *d_converged, int check_voxels,
                                      uint64_t *d_valid_bits, uint8_t *d_flags, void *stream);

/* ---- motion validity: MotionValidator::checkMotion -------------------------------------- */

typedef struct {
  double min_tension_change;     /* motion-planning/Problem.h:59 (0.02)   */
  double min_rotation_change;    /* :61 (0.01)                            */
  double min_retraction_change;  /* :62 (0.0001)                          */
} tr_space_params;

/* Batched AbstractVoxelMotionValidator::checkMotion(s1, s2)
 * (motion-planning/AbstractVoxelMotionValidator.h:143-151 -> VoxelBackboneMotionValidator.cpp:41-81
 * -> VoxelEnvironment::voxelize_valid_backbone_motion, VoxelEnvironment.cpp:207-444), replacing
 * the loops at VoxelCachedLazyPRM.cpp:1520-1542 and :1621-1641.  a, b: n_edges x S host states.
 * n_fk (optional) receives the number of FK samples taken per edge.
 * An edge whose samples leave the voxel domain (std::domain_error in the reference) is reported
 * invalid and counted in *n_domain_errors (optional). */
int tr_validate_edges(tr_ctx *ctx, const tr_space_params *sp, const double *a, const double *b,
                      int64_t n_edges, uint64_t *valid_bits, int32_t *n_fk, int64_t *n_domain_errors);

/* The same for a roadmap: edge e joins states[edges[2e]] and states[edges[2e + 1]] (rows of one n_states x S
 * array, the graph's vertices).  Every vertex is evaluated once for all of its edges -- the reference's
 * checkMotion recomputes both end shapes for every edge (VoxelEnvironment.cpp:262-272) -- with identical
 * verdicts and n_fk (which keeps counting the two ends per edge, as the reference does). */
int tr_validate_edges_indexed(tr_ctx *ctx, const tr_space_params *sp, const double *states, int64_t n_states,
                              const int32_t *edges, int64_t n_edges, uint64_t *valid_bits, int32_t *n_fk,
                              int64_t *n_domain_errors);

/* Batched checkMotion(s1, s2, last_valid) (AbstractVoxelMotionValidator.h:153-169 ->
 * voxelize_until_invalid, VoxelBackboneMotionValidator.cpp:83-91): same verdict bits, plus per edge
 * last_valid_t = PartialVoxelization::t, the largest sampled interpolation parameter below the first
 * invalid sample (1.0 for a valid edge, 0.0 when already the start is invalid).  The caller obtains
 * last_valid.first with its own space->interpolate(s1, s2, t).  A sample is judged by the installed state
 * checker (tr_set_checker), as voxelize_until_invalid_impl does. */
int tr_validate_edges_last_valid(tr_ctx *ctx, const tr_space_params *sp, const double *a, const double *b,
                                 int64_t n_edges, uint64_t *valid_bits, double *last_valid_t, int32_t *n_fk);

/* Batched discrete edge check: VoxelBackboneDiscreteMotionValidator::generic_voxelize
 * (motion-planning/VoxelBackboneDiscreteMotionValidator.cpp:9-79, the loop of
 * ompl::base::DiscreteMotionValidator::checkMotion): samples a, interpolate(i / nd) for
 * i = 1 .. nd-1 with nd = validSegmentCount(a, b), then b; the edge is valid iff every sample is a
 * valid state.  last_valid_t (optional) = PartialVoxelization::t, n_fk (optional) = samples the
 * reference's sequential loop evaluates (it stops after the first invalid one).  With last_valid_t the call is
 * checkMotion(s1, s2, last_valid) and a sample is judged by the installed state checker; without it the call is
 * checkMotion(s1, s2): shape validity per sample plus the swept backbone volume (see tr_set_checker). */
int tr_validate_edges_discrete(tr_ctx *ctx, const tr_space_params *sp, const double *a, const double *b,
                               int64_t n_edges, uint64_t *valid_bits, double *last_valid_t, int32_t *n_fk);

/* ---- loaded edges: checkMotion with every FK sample taken from TendonRobot::general_shape --- */

/* The reference's motion validator takes every sample's shape from _vc->fk(state) (motion-planning/
 * VoxelBackboneMotionValidator.cpp:25), and AbstractValidityChecker::set_fk_func swaps that FK for general_shape under a
 * load (apps/profile_chained_plan.cpp:407-451): checkMotion then bisects on loaded shapes.  These calls are that, for a
 * batch of edges and ONE load set per call. */
enum { TR_LOAD_FRAME_BASE = 0, TR_LOAD_FRAME_WORLD = 1 };
typedef struct tr_edge_loads {
  double wrench[6];    /* F_e, L_e */
  double dist[6];      /* f_e, l_e per unit length */
  int32_t frame;       /* BASE: tr_fk_loaded_batch's frame (before the state's rotation), the same 12 numbers for every sample.
                          WORLD: fixed in the frame after rotate_z; a sample with rotation theta gets Rz(-theta) applied to all
                          four vectors (robots without rotation: the same as BASE) */
  int32_t warm_start;  /* 0: every sample starts from the unloaded solution of its tensions (tr_fk_loaded_batch without a guess).
                          1: a midpoint starts from the accepted base strains of its interval's sample at t_a; the end states
                          (the indexed form's vertices) start cold */
} tr_edge_loads;

/* tr_validate_edges (last_valid_t == NULL: checkMotion(s1, s2)) or tr_validate_edges_last_valid (otherwise:
 * checkMotion(s1, s2, last_valid)) on loaded shapes: the same level-synchronous bisection, sample tests, verdict bits, n_fk and
 * last_valid_t, every sample solved by the shooting of tr_fk_loaded_batch with `shoot` (NULL: its defaults) and the sample's
 * loads.  A sample whose shooting does not converge is an INVALID sample (general_tension_shape sets res.converged = false and
 * is_valid_shape rejects it), never an error of the call.  loads == NULL: no load, cold start.
 *   n_unconverged   (optional) samples whose shooting did not converge
 *   n_integrations  (optional) the sum of the samples' fk_calls (tr_fk_loaded_batch's fk_calls_out)
 * The rotation of WORLD loads uses a fixed sequence of IEEE operations for sine and cosine (csrc/loaded_edge_kernel.hpp), so a
 * host restatement reproduces the per-sample rows bit for bit.  No grid or a
 * non-positive resolution: TR_ERR_INVALID_ARG; n_edges == 0: TR_OK.  The verdicts do not depend on the chunking
 * (TENDON_HIP_SHOOT_CHUNK, TENDON_HIP_EDGE_POOL), the order of the edges or the other edges of the call.
 * Robots with retraction: TR_ERR_UNSUPPORTED unless the context is at TR_LOADED_RETRACTION_EDGES (tr_set_loaded_retraction).  Then
 *   - a sample's state is the unloaded edge check's interpolation, s_start linear;
 *   - its shape is tr_fk_loaded_batch's for that state: its own grid t_range(s_start, L, dL), rows aligned at the tip, the sample's
 *     own loads under frame WORLD;
 *   - it is valid if it converged, its lengths are within the limits against home_shape(s_start).L_i, it has no self collision and
 *     it passes the sample test the run chose (the sphere checker under last_valid_t included);
 *   - s_start >= L: one point at the origin, converged, judged as the unloaded stored-point check of such a robot judges that shape;
 *     s_start < 0: unconverged, so invalid;
 *   - the interval test compares stored points with the samples' own point counts, as the unloaded voxelize forms of such a robot do;
 *   - warm_start is allowed: the guess is the accepted base strains of the interval's sample at t_a, unchanged -- strains at another
 *     arc length, a heuristic about which nothing is promised. */
int tr_validate_edges_loaded(tr_ctx *ctx, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                             const double *a, const double *b, int64_t n_edges, uint64_t *valid_bits, double *last_valid_t,
                             int32_t *n_fk, int64_t *n_domain_errors, int64_t *n_unconverged, int64_t *n_integrations);
/* The roadmap form (tr_validate_edges_indexed's arguments and n_fk convention): every vertex is solved and swept once, cold, for
 * all of its edges; with warm_start its accepted strains start the first midpoints of its edges. */
int tr_validate_edges_loaded_indexed(tr_ctx *ctx, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                     const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges,
                                     uint64_t *valid_bits, int32_t *n_fk, int64_t *n_domain_errors, int64_t *n_unconverged,
                                     int64_t *n_integrations);
/* The accepted base strains (v0, u0), n_states x 6, of the vertices of the context's last tr_validate_edges_loaded_indexed call:
 * tr_fk_loaded_batch's vu0_out for the same states and per-state loads.  TR_ERR_INVALID_ARG when none are resident (no indexed
 * call yet, a pairwise loaded call since, the call took the pairwise form) or n_states is not that call's. */
int tr_edges_loaded_vertex_strains(tr_ctx *ctx, int64_t n_states, double *vu0_out);
/* How the context's last loaded edge call ran (tuning, benchmarks): samples evaluated (those of chunks retried after a pool
 * overflow included), levels (one loads / guess / shooting / K2 sequence each), Levenberg-Marquardt rounds (one host
 * synchronisation each), chunk attempts. */
int tr_edges_loaded_last(const tr_ctx *ctx, int64_t stats[4]);

/* ---- the roadmap build on loaded shapes -------------------------------------------------- */

/* In the reference set_fk_func(general_shape ...) changes createRoadmap's vertex loop, voxelizeVertex and voxelizeEdge at once,
 * because they all take their shapes from voxelStateChecker_->fk (motion-planning/VoxelCachedLazyPRM.cpp:1415-1439, 2803-2837,
 * 2879-2902).  These calls are those loops on the loaded FK.  shoot == NULL: the solver's defaults; loads == NULL: no load.  Every
 * vertex is solved cold, so it has the same strains, points and tip -- bit for bit -- in the vertex phase, in
 * tr_voxelize_batch_loaded, as an end state of the indexed edge calls and in tr_fk_loaded_batch with the per-state load rows.
 * All report n_unconverged and n_integrations as the loaded edge calls do (optional).  Robots with retraction:
 * TR_ERR_UNSUPPORTED; a bad frame or no grid: TR_ERR_INVALID_ARG; an empty call: TR_OK before the grid is asked for. */

/* tr_sample_valid_vertices on loaded shapes: the accepted set is the first n_want candidates i of the sequence (seed, first_candidate
 * + i) whose loaded shape -- tr_fk_loaded_batch's, cold, under the candidate's load rows (BASE or WORLD) -- is valid under the
 * installed checker; an unconverged candidate is an invalid one.  A pure function of (seed, first_candidate, box, loads, shoot): it
 * does not depend on the batch size or on TENDON_HIP_SHOOT_CHUNK.  vu0 (optional): n_want x 6, the accepted base strains.
 * n_unconverged / n_integrations: sums over the n_tried candidates consumed.  Each batch of candidates is generated, loaded, solved,
 * swept and compacted on the device; the host reads one counter block per batch. */
int tr_sample_valid_vertices_loaded(tr_ctx *ctx, const tr_shoot_params *shoot, const tr_edge_loads *loads, uint64_t seed,
                                    uint64_t first_candidate, const double *lo, const double *hi, int64_t n_want, int64_t max_candidates,
                                    double *states, double *tips, int64_t *index, double *vu0, int64_t *n_accepted, int64_t *n_tried,
                                    int64_t *n_unconverged, int64_t *n_integrations);
/* ... with device outputs (d_tips, d_index, d_vu0 optional).  The run is the null stream's and ends synchronised. */
int tr_sample_valid_vertices_loaded_dev(tr_ctx *ctx, const tr_shoot_params *shoot, const tr_edge_loads *loads, uint64_t seed,
                                        uint64_t first_candidate, const double *lo, const double *hi, int64_t n_want,
                                        int64_t max_candidates, double *d_states, double *d_tips, int64_t *d_index, double *d_vu0,
                                        int64_t *n_accepted, int64_t *n_tried, int64_t *n_unconverged, int64_t *n_integrations,
                                        void *stream);
/* tr_voxelize_batch (voxelizeVertex: shape validity, block list, tip) on loaded shapes, cold start; the same CSR and the
 * tr_voxelize_fetch* protocol. */
int tr_voxelize_batch_loaded(tr_ctx *ctx, const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *states, int64_t n,
                             int64_t *offsets, uint64_t *shape_valid_bits, double *tips, int64_t *n_unconverged,
                             int64_t *n_integrations);
/* tr_voxelize_edges_indexed / tr_connect_edges_indexed on loaded samples: tr_validate_edges_loaded_indexed's bisection (warm_start
 * honoured the same way) with the voxelize forms' sample tests and block lists.  tr_edges_loaded_vertex_strains and
 * tr_edges_loaded_last also answer for these calls. */
int tr_voxelize_edges_loaded_indexed(tr_ctx *ctx, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                     const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges, int64_t *offsets,
                                     uint64_t *fully_valid_bits, int32_t *n_fk, int64_t *n_unconverged, int64_t *n_integrations);
int tr_connect_edges_loaded_indexed(tr_ctx *ctx, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                    const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges, int64_t *offsets,
                                    uint64_t *valid_bits, int32_t *n_fk, int64_t *n_unconverged, int64_t *n_integrations);
/* The tips of loaded shapes alone: tr_fk_loaded_batch's shooting (`shoot`, NULL: its defaults; wrench / dist rows and `guess` as
 * there, NULL guess: cold) and fk_shape.p.back() of the integration at the final strains -- bit for bit tr_fk_loaded_batch's last
 * point, tr_voxelize_batch_loaded's tip and the loaded vertex phase's.  The shapes are integrated into the context's point workspace
 * a chunk at a time, so no plane is ever n columns wide.
 *   tips n x 3, converged n, vu0 n x 6 (the accepted base strains) -- all optional
 *   rounds_out  optional int64[2]: shooting rounds (one host synchronisation each), the sum of the problems' integrations
 * A state whose shooting does not converge has converged = 0 and the tip of its last strains: never an error of the call.  Robots with
 * retraction: TR_ERR_UNSUPPORTED, or, on a context opened by tr_set_loaded_retraction, taken as tr_fk_loaded_batch takes them
 * (s_start >= L or < 0: the origin); n == 0: TR_OK.  The _dev form takes device arrays; its run is the null stream's (the device is
 * drained before it) and ends synchronised.  A state's result does not depend on the batch or on TENDON_HIP_SHOOT_CHUNK. */
int tr_fk_loaded_tips(tr_ctx *ctx, const tr_shoot_params *shoot, const double *states, int64_t n, const double *wrench, int64_t wrench_ld,
                      const double *dist, int64_t dist_ld, const double *guess, double *tips, uint8_t *converged, double *vu0,
                      int64_t *rounds_out);
int tr_fk_loaded_tips_dev(tr_ctx *ctx, const tr_shoot_params *shoot, const double *d_states, int64_t n, const double *d_wrench,
                          int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess, double *d_tips,
                          uint8_t *d_converged, double *d_vu0, int64_t *rounds_out, void *stream);

/* ---- tip inverse kinematics on loaded shapes --------------------------------------------- */

/* tip_control::inverse_kinematics (tip-control/tip_control.cpp:35-140) takes any FKFunc; with TendonRobot::general_shape installed
 * it solves for the tip of the LOADED shape.  These calls are tr_ik_batch for that case: the same projected Levenberg-Marquardt on
 * the state, bounds, stop tests and canonical rotation (`params`, NULL: tr_ik_batch's defaults), under ONE load set per call
 * (`loads`, tr_edge_loads' meaning of BASE and WORLD; NULL: no load; warm_start is not read).
 * The tip Jacobian is not differenced through shooting solves.  At base strains y that balance the tip, e_w(y, p) = 0, the tip
 * x(y, p) moves with the state as dx/dp = X_p - X_y J_y^-1 J_p; the four blocks are central differences of 13 + 2 S integrations
 * from one point (the state's steps are levmar's max(|1e-4 p|, delta), the strains' the shooting's finite_difference_delta itself).
 * Per outer round every active problem's trial state is equilibrated by tr_fk_loaded_batch's shooting (`shoot`, NULL: its defaults
 * with stop_threshold_Dp = 0 -- the steps from a predicted start are small by construction) from the predicted strains y - J_y^-1 J_p (p_trial - p); a trial whose shooting does not converge is a
 * rejected step, a start whose shooting does not converge ends its problem (equilibrium = 0, error = inf, tip = NaN).
 *   initial_states  n x S, clipped to the bounds;  des: goals, row i at des + i des_ld (des_ld = 0: one goal for all)
 *   lo, hi          S bounds each, or NULL: Bounds::from_robot
 *   guess           optional n x 6 start strains (v0, u0) of the starts' shooting (NULL: the unloaded solution)
 *   states_out n x S, tips_out n x 3 (the loaded tip at states_out), error_out n (|des - tip|), iters_out n (outer iterations),
 *   fk_calls_out n (integrations: the shooting's and the 13 + 2 S per round), vu0_out n x 6 (the base strains of the returned
 *   state's equilibrium: tr_fk_loaded_batch's `guess` for it), equilibrium_out n -- all optional
 *   rounds_out      optional int64[2]: outer rounds, shooting rounds (one host synchronisation each)
 * Robots with retraction: TR_ERR_UNSUPPORTED; a bad frame or lo > hi: TR_ERR_INVALID_ARG; n == 0: TR_OK.  A problem's result does
 * not depend on the batch size, the order, the chunking (TENDON_HIP_SHOOT_CHUNK) or the other problems of the call. */
int tr_ik_loaded_batch(tr_ctx *ctx, const tr_ik_params *params, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                       const double *initial_states, int64_t n, const double *des, int64_t des_ld, const double *lo, const double *hi,
                       const double *guess, double *states_out, double *tips_out, double *error_out, int32_t *iters_out,
                       int32_t *fk_calls_out, double *vu0_out, uint8_t *equilibrium_out, int64_t *rounds_out);
/* ... with device arrays (lo, hi and rounds_out stay host pointers); the run is ordered on `stream` and ends synchronised. */
int tr_ik_loaded_batch_dev(tr_ctx *ctx, const tr_ik_params *params, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                           const double *d_initial_states, int64_t n, const double *d_des, int64_t des_ld, const double *lo,
                           const double *hi, const double *d_guess, double *d_states_out, double *d_tips_out, double *d_error_out,
                           int32_t *d_iters_out, int32_t *d_fk_calls_out, double *d_vu0_out, uint8_t *d_equilibrium_out,
                           int64_t *rounds_out, void *stream);

/* ---- tip Jacobian and tip compliance of loaded shapes ------------------------------------- */

/* tr_tip_jacobian for LOADED shapes: the linearisation the loaded IK forms in every round of its loop, for n states in one call.
 * It replaces differencing tr_fk_loaded_batch through 2 S + 1 shooting solves per state (each with its own stopping noise) by one
 * solve and 13 + 2 S integrations.  Every state is equilibrated by tr_fk_loaded_batch's shooting (`shoot`, NULL: its defaults;
 * `guess`: optional n x 6 start strains, NULL: the unloaded solution) under ONE load set per call (`loads`, tr_edge_loads' meaning
 * of BASE and WORLD; NULL: no load; warm_start is not read).  With max_iters = 0 and a guess the state is linearised exactly at
 * the guess: one integration, equilibrium = (residual <= residual_threshold) as tr_fk_loaded_batch defines it.
 * At base strains y with e_w(y, p) = balance(y, p) - w = 0 and the blocks J_y = de_w/dy, J_p = de_w/dp, X_y = dx/dy, X_p = dx/dp
 * (central differences; the state's steps are levmar's max(|1e-4 p_k|, delta), the strains' the shooting's
 * finite_difference_delta itself):
 *   W = J_y^-1 J_p                  n x 6 x S   (-W = dy/dp: the loaded IK's strain predictor)
 *   J = X_p - X_y W                 n x 3 x S   dx/dp, the tip Jacobian of the loaded shape -- bit for bit the loaded IK's
 *   compliance = X_y J_y^-1 T       n x 3 x 6   dx/dw: tip displacement per unit tip force and moment, with respect to the wrench AS
 *                                               GIVEN: T = I (BASE), blockdiag(Rz(-theta), Rz(-theta)) (WORLD on a robot with rotation)
 *   vu0 = y - J_y^-1 e_w            n x 6       the strains after one Newton step (the shooting stops at the threshold)
 *   tips = x - X_y J_y^-1 e_w       n x 3       the tip there
 *   equilibrium                     n           the shooting converged (and J_y has no zero pivot)
 *   blocks                          n x (69 + 9 S), row-major each: y(6), x(3), e_w(6), J_y(36), J_p(6 S), X_y(18), X_p(3 S) --
 *                                               what the results above were reduced from
 *   n_integrations                  n           the shooting's integrations and the 13 + 2 S lanes
 *   rounds_out                      one int64: shooting rounds (one host synchronisation each)
 * All outputs are optional.  A state whose shooting does not converge has equilibrium = 0 and NaN in every double output: never
 * an error of the call.  A zero pivot of J_y leaves inf / NaN in what is solved with it.
 * Robots with retraction: TR_ERR_UNSUPPORTED; a bad frame, delta <= 0 or null states: TR_ERR_INVALID_ARG; n == 0: TR_OK.  A
 * problem's result does not depend on the batch size, the order, the chunking (TENDON_HIP_SHOOT_CHUNK) or the other problems. */
int tr_tip_jacobian_loaded(tr_ctx *ctx, const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *states, int64_t n,
                           double delta, const double *guess, double *tips, double *J, double *compliance, double *W, double *vu0,
                           uint8_t *equilibrium, double *blocks, int64_t *n_integrations, int64_t *rounds_out);
/* ... with device arrays (rounds_out stays a host pointer); the run is ordered on `stream` and ends synchronised. */
int tr_tip_jacobian_loaded_dev(tr_ctx *ctx, const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *d_states,
                               int64_t n, double delta, const double *d_guess, double *d_tips, double *d_J, double *d_compliance,
                               double *d_W, double *d_vu0, uint8_t *d_equilibrium, double *d_blocks, int64_t *d_n_integrations,
                               int64_t *rounds_out, void *stream);

/* ---- cached voxel sets vs obstacles: VoxelOctree::collides on roadmap caches ------------ */

/* Batched `obstacles.collides(*cached_voxels)` for roadmap vertices / edges
 * (motion-planning/VoxelCachedLazyPRM.cpp:2397-2411, :2497-2509, :2607-2631).  Items are sparse
 * block lists in CSR form: item i owns entries offsets[i]..offsets[i+1]-1 of (block_ids, masks);
 * block id = ((bx*Nb)+by)*Nb+bz.  hit_bits: ceil(n_items/64) words, bit set = collides. */
int tr_check_cached(tr_ctx *ctx, const uint32_t *block_ids, const uint64_t *masks,
                    const int64_t *offsets, int64_t n_items, uint64_t *hit_bits);
int tr_check_cached_dev(tr_ctx *ctx, const uint32_t *d_block_ids, const uint64_t *d_masks,
                        const int64_t *d_offsets, int64_t n_items, uint64_t *d_hit_bits, void *stream);

/* The same test for a SUBSET of the items: d_list[q] names an item, d_hit[q] (one byte) receives its verdict.
 * The lazy query loop (tr_roadmap_solve) validates the unknown items of all candidate paths of a round with one
 * launch of this -- the batched form of computeVertexValidity / computeEdgeValidity on cached sets
 * (motion-planning/VoxelCachedLazyPRM.cpp:2607-2631). */
int tr_check_cached_subset_dev(tr_ctx *ctx, const uint32_t *d_block_ids, const uint64_t *d_masks,
                               const int64_t *d_offsets, int64_t n_items, const int32_t *d_list, int64_t n_list,
                               uint8_t *d_hit, void *stream);

/* ---- robot voxel sets for roadmap caches: voxelizeVertex / voxelizeEdge -------------------------- */

/* Batched VoxelCachedLazyPRM::voxelizeVertex (motion-planning/VoxelCachedLazyPRM.cpp:2803-2837),
 * replacing the loop at :1704-1713: FK, is_valid_shape (no obstacle test), and for every valid shape
 * the voxel set voxelize_impl would return (VoxelBackboneValidityChecker.h:49-57) as a sparse list
 * of (block id, mask).  Results are CSR: offsets[n+1] is written here (item i owns
 * offsets[i]..offsets[i+1]-1, nothing for an invalid shape); the lists stay inside the context
 * until tr_voxelize_fetch copies them.  shape_valid_bits: ceil(n/64) words; tips optional n x 3.
 * Inside an item the blocks are distinct and ordered by block id. */
int tr_voxelize_batch(tr_ctx *ctx, const double *states, int64_t n, int64_t *offsets,
                      uint64_t *shape_valid_bits, double *tips);

/* Batched VoxelCachedLazyPRM::voxelizeEdge (:2879-2902 -> AbstractVoxelMotionValidator::voxelize,
 * AbstractVoxelMotionValidator.h:98-107), replacing the loop at :1751-1775: the swept-volume
 * voxelisation of every edge whose samples are all shape-valid (is_fully_valid); other edges get an
 * empty item and a 0 bit.  Same CSR + fetch protocol. */
int tr_voxelize_edges(tr_ctx *ctx, const tr_space_params *sp, const double *a, const double *b,
                      int64_t n_edges, int64_t *offsets, uint64_t *fully_valid_bits, int32_t *n_fk);

/* The same for a roadmap: edge e joins states[edges[2e]] and states[edges[2e + 1]]; every vertex is integrated and
 * voxelised ONCE for all of its edges (the loop at :1751-1775 recomputes both end shapes per edge).  Same sets. */
int tr_voxelize_edges_indexed(tr_ctx *ctx, const tr_space_params *sp, const double *states, int64_t n_states,
                              const int32_t *edges, int64_t n_edges, int64_t *offsets, uint64_t *fully_valid_bits,
                              int32_t *n_fk);

/* connectVertices and voxelizeEdge in one pass (createRoadmap adds an edge when checkMotion accepts it, :1491-1502, and
 * voxelises it, :1751-1775 -- two traversals of the same samples): the samples are tested against the obstacle grid as
 * tr_validate_edges_indexed tests them AND voxelised as tr_voxelize_edges_indexed voxelises them.  valid_bits are
 * checkMotion's verdicts; a valid edge owns the voxel set tr_voxelize_edges_indexed gives it, an invalid one nothing. */
int tr_connect_edges_indexed(tr_ctx *ctx, const tr_space_params *sp, const double *states, int64_t n_states,
                             const int32_t *edges, int64_t n_edges, int64_t *offsets, uint64_t *valid_bits, int32_t *n_fk);

/* The block lists of the last tr_voxelize_* call stay in device memory (they are produced there, and their consumers --
 * tr_check_cached_dev, tr_roadmap_set_caches_dev -- read them there); capacity must be >= its offsets[n] = tr_voxelize_count.
 * tr_voxelize_fetch copies them to host arrays; tr_voxelize_fetch_dev copies them device to device into arrays the caller
 * owns (complete when it returns; the next tr_voxelize_* call overwrites the store). */
int tr_voxelize_fetch(tr_ctx *ctx, uint32_t *block_ids, uint64_t *masks, int64_t capacity);
int tr_voxelize_fetch_dev(tr_ctx *ctx, uint32_t *d_block_ids, uint64_t *d_masks, int64_t capacity, void *stream);
int64_t tr_voxelize_count(const tr_ctx *ctx);

/* ---- nearest neighbours in state space ---------------------------- */

/* For every state its k nearest among the same n states in the reference's state-space metric
 * (CompoundStateSpace::distance with the subspace weights of motion-planning/Problem.cpp:112-152):
 * the neighbour lists connectionStrategy_(v) produces in createRoadmap phase 3
 * (motion-planning/VoxelCachedLazyPRM.cpp:1491-1502; KBoundedStrategy :1339 / KStarStrategy :1352).
 * Like nearestK on a structure that already contains v, row i starts with i itself at distance 0.
 * Entries farther than max_distance (KBoundedStrategy's bound; pass INFINITY for none) are -1 / inf.
 * idx, dist: n x k row-major, ascending distance.  Exact: every pair is either computed or excluded by a bound on one coordinate. */
int tr_knn(tr_ctx *ctx, const double *states, int64_t n, int32_t k, double max_distance,
           int32_t *idx, double *dist);

/* Layout and metric of the state space built by motion_planning::Problem::create_space_information
 * (motion-planning/Problem.cpp:101-163): number of tension dimensions, whether a rotation / retraction coordinate
 * follows, and the weights of those two subspaces in CompoundStateSpace::distance (tension weight 1). */
int tr_state_layout(const tr_ctx *ctx, int32_t *n_tendons, int32_t *has_rotation, int32_t *has_retraction);
int tr_space_weights(const tr_ctx *ctx, double *w_rotation, double *w_retraction);

/* ---- interactive queries on a cached roadmap (BASELINE config 5) -------------------------------------
 * motion_planning::VoxelCachedLazyPRM::solveWithRoadmap / constructSolution
 * (motion-planning/VoxelCachedLazyPRM.cpp:1977-2096, :2689-2771) for a BATCH of (start, goal) vertex pairs:
 * A* with the state-space distance as heuristic (astarSearch :2950-2976, costHeuristic :2773-2775) on the host
 * cores, validity of the candidate paths' vertices and edges from their cached voxel sets -- resident in HBM --
 * with one K4 launch per round over all queries' unknown items (computeVertexValidity / computeEdgeValidity
 * :2607-2631), invalid items leave the graph (removeVertices / removeEdge), repeat until every query has a valid
 * path or its start and goal are disconnected.  Accepted paths equal the reference's (equal cost; equal vertex
 * sequence unless two paths tie exactly).  The roadmap object borrows `ctx` (obstacle grid, device) and must be
 * destroyed before it. */
typedef struct tr_roadmap tr_roadmap;
typedef struct {
  int64_t rounds;          /* search / validate rounds of the last solve                        */
  int64_t items_checked;   /* cached sets tested against the obstacle grid (K4 work)            */
  int64_t astar_runs;      /* A* searches (>= queries: a query searches again after removals)    */
  int64_t expanded;        /* vertices taken off the open lists                                  */
} tr_roadmap_stats;
#define TR_QUERY_SOLVED        0
#define TR_QUERY_NO_PATH       1   /* start and goal are in different components (solveWithRoadmap :2026-2036) */
#define TR_QUERY_INVALID_START 2   /* ob::PlannerStatus::INVALID_START (solvePrep :2995-2998)                  */
#define TR_QUERY_INVALID_GOAL  3
/* Graph of a loaded roadmap (fromRoadmapParser :2357-2580): n_vertices x S states, n_edges index pairs,
 * edge weights (weightProperty_; NULL = state-space distance, what connectVertices stores :2857-2861). */
int tr_roadmap_create(tr_ctx *ctx, const double *states, int64_t n_vertices, const int32_t *edges,
                      const double *weights, int64_t n_edges, tr_roadmap **out);
/* Device buffers of a destroyed (or re-attached) roadmap are parked in a per-process cache for the next one -- at most 3 GiB /
 * 48 buffers; a failed allocation empties it first -- so free device memory does not return to its earlier level at once. */
void tr_roadmap_destroy(tr_roadmap *rm);
const char *tr_roadmap_last_error(const tr_roadmap *rm);
/* Upload the cached voxel sets (vertexVoxelsProperty_ / edgeVoxelsProperty_) as CSR block lists -- the output of
 * tr_voxelize_batch / tr_voxelize_edges* or of a .rmp file.  present bits (optional): a 0 bit = no cache, because
 * voxelizeVertex / voxelizeEdge found the shape invalid (:2803-2837, :2879-2902): such an item is invalid in every
 * environment. */
int tr_roadmap_set_caches(tr_roadmap *rm, const int64_t *v_offsets, const uint32_t *v_block_ids, const uint64_t *v_masks,
                          const uint64_t *v_present_bits, const int64_t *e_offsets, const uint32_t *e_block_ids,
                          const uint64_t *e_masks, const uint64_t *e_present_bits);
/* The same with the block ids / masks in device memory (the arrays tr_voxelize_fetch_dev filled): the caches of a roadmap
 * built on this GPU never cross PCIe.  Offsets and present bits are host arrays as above. */
int tr_roadmap_set_caches_dev(tr_roadmap *rm, const int64_t *v_offsets, const uint32_t *d_v_block_ids, const uint64_t *d_v_masks,
                              const uint64_t *v_present_bits, const int64_t *e_offsets, const uint32_t *d_e_block_ids,
                              const uint64_t *d_e_masks, const uint64_t *e_present_bits);
/* Landmark tables for the searches of tr_roadmap_solve: graph distances from n_landmarks extremal vertices over ALL edges
 * (one Dijkstra each, on n_threads host threads; 0 = the process's CPU share).  They sharpen A*'s heuristic -- the
 * reference's state-space distance (costHeuristic :2773-2775) -- by lower bounds that stay valid when invalid items leave
 * the graph, so the returned paths and costs are unchanged and far fewer vertices are expanded.  n_landmarks = 0 searches
 * with the reference's heuristic alone.  Without this call the first tr_roadmap_solve of >= 64 queries builds 16. */
int tr_roadmap_prepare(tr_roadmap *rm, int32_t n_landmarks, int32_t n_threads);
/* clearValidity (:1656-1663): everything unknown again, removed items back in the graph -- call it after the
 * obstacle grid of `ctx` changed (tr_set_grid / tr_grid_*). */
int tr_roadmap_clear_validity(tr_roadmap *rm);
/* Eager form of the loading loops (:2397-2411, :2486-2526): every cached set against the current grid in one K4
 * launch; afterwards no query finds an unknown item. */
int tr_roadmap_revalidate(tr_roadmap *rm, int64_t *n_invalid_vertices, int64_t *n_invalid_edges);
/* status per item: 0 unknown, 1 valid, 2 invalid (removed) */
int tr_roadmap_get_validity(tr_roadmap *rm, uint8_t *vertex_status /*[n_vertices]*/, uint8_t *edge_status /*[n_edges]*/);
/* The inverse of tr_roadmap_get_validity: what a builder already knows goes in (either array may be NULL = leave as it is).
 * createRoadmap with ValidateVertices / ValidateEdges leaves the items it accepted VALIDITY_TRUE
 * (vertexValidityProperty_ :1476, computeEdgeValidity :2621-2631), so the first query on such a roadmap tests nothing again. */
int tr_roadmap_set_validity(tr_roadmap *rm, const uint8_t *vertex_status /*[n_vertices]*/, const uint8_t *edge_status /*[n_edges]*/);
/* The batched query loop (lazy: only the items on candidate paths are tested, round by round -- until so many queries are still
 * open after a round that testing every cached set at once is cheaper than another round, see TENDON_HIP_LAZY_ONLY).  status[q] = TR_QUERY_*; cost[q] (optional) = path cost; path_offsets[n_queries + 1]:
 * query q's path (start ... goal) is entries path_offsets[q] .. path_offsets[q+1]-1 of the array
 * tr_roadmap_fetch_paths copies out.  n_threads = host threads for the A* searches (0 = the process's CPU share).
 * Validity discovered by a call is kept for the next one (as the reference's graph keeps it between queries). */
int tr_roadmap_solve(tr_roadmap *rm, const int32_t *starts, const int32_t *goals, int64_t n_queries, int32_t n_threads,
                     int32_t *status, double *cost, int64_t *path_offsets, tr_roadmap_stats *stats);
int tr_roadmap_fetch_paths(tr_roadmap *rm, int32_t *path_vertices, int64_t capacity);
/* Where the graph searches of the last tr_roadmap_solve ran (the A* of a round is done by the `roadmap_astar` kernel, one wave
 * per query, when the round has 512 queries or more -- see TENDON_HIP_SEARCH below -- and by the host threads otherwise; the
 * answers are the same):  out[0] searches finished by the kernel, out[1] searches the kernel handed back to the host threads
 * (over its pop budget, or a list full), out[2] searches the host threads took while the kernel ran (the ones expected to be
 * longest), out[3] times a search's open list moved entries between its LDS part and its HBM part, out[4] vertex expansions
 * by the kernel (those of searches it handed back included), out[5] vertex expansions by the host threads, out[6] queries answered
 * "no path" without a search because their end points lie in different components of the roadmap minus the items known invalid
 * (the reference's solutionComponent test, :2015-2044; labels recomputed on the device per round, see TENDON_HIP_COMPONENTS), out[7] times
 * a search on the device outgrew its table of per-vertex records and moved into a larger one from the shared pool. */
int tr_roadmap_search_stats(tr_roadmap *rm, int64_t out[8]);
/* The roadmap_astar launches of the last tr_roadmap_solve, timed with HIP events on the stream they ran on: out[0] their total
 * milliseconds, out[1] their number, out[2] the vertex expansions they did, out[3] the ALGORITHMIC bytes of one expansion on this
 * roadmap (the vertex's record and row header, and per arc: the arc, two validity bytes, the arc count, the neighbour's record read
 * and written, its state and landmark rows) -- bench.py turns them into the kernel's HBM roofline fraction. */
int tr_roadmap_profile(tr_roadmap *rm, double out[4]);
/* The device searches' state -- a table of per-vertex records per search in flight, a pool of larger ones, the per-round arrays: sized
 * by the largest round so far (a 512-query round ~0.9 GB, 3 072 searches in flight ~5.3 GB, whatever the roadmap's size), it stays with the
 * roadmap between calls.  tr_roadmap_release_search_state hands it back to the device (the adjacency rows stay; the next round of 512
 * queries or more allocates tables again, ~2 ms) and reports the bytes; tr_roadmap_search_state_bytes says what is held now.  When an
 * allocation anywhere in the library runs out of device memory, the tables of every roadmap that is not inside a call are released
 * the same way before the allocation is tried again. */
int tr_roadmap_release_search_state(tr_roadmap *rm, int64_t *bytes_released);
/* ... and setting it up ahead of the first batch (the adjacency rows and the tables for rounds of up to n_queries queries: a process's first
 * allocation of the full 5.3 GB takes ~0.15 s, which otherwise falls into the first tr_roadmap_solve of 512 queries or more).
 * TR_ERR_UNSUPPORTED when this roadmap's searches stay on the host threads (parallel edges, state size above the kernel's, no memory). */
int tr_roadmap_reserve_search_state(tr_roadmap *rm, int64_t n_queries);
/* Searches of the last tr_roadmap_solve that were answered by a parallel SWEEP on the device instead of A*: a host search that passes a
 * sixth of the graph in expansions (50 000 at least; TENDON_HIP_SEARCH_SWEEP=n overrides, 0 = never) is abandoned and its source's
 * distances are relaxed over all valid arcs at once until nothing changes -- the same cost bit for bit, the path walked back along
 * arcs that meet it exactly.  Only on roadmaps whose searches are set up on the device (a round of 512 queries or more has run, or
 * tr_roadmap_reserve_search_state). */
int tr_roadmap_search_sweeps(tr_roadmap *rm, int64_t *n);
int tr_roadmap_search_state_bytes(tr_roadmap *rm, int64_t *bytes);

/* ---- tip-goal queries on a cached roadmap: roadmapIk + solveWithRoadmap for a batch ----------------------
 * The reference's interactive loop (apps/roadmap_chained_plan.cpp:535-679) asks, per waypoint, roadmapIk(goal_tip, tol, k, opts)
 * (motion-planning/VoxelCachedLazyPRM.cpp:3095-3577) and then solveWithRoadmap.  Here n requests go through both in one call, with
 * the roadmap's tips, states and validity bytes resident in HBM.  For request q (tip r_q, start vertex s_q):
 *   1. N_q = the first k vertices in the order (d2, vertex index) among the vertices that have a tip and are valid in the current
 *      grid (exactly what tr_roadmap_revalidate reports; a vertex without a cache is invalid), d2 = ((tx-rx)^2 + (ty-ry)^2) +
 *      (tz-rz)^2 in fp64 without contraction; a row with fewer than k is padded with -1; none: TR_TIPQ_NO_NEIGHBOR.  Vertex
 *      validity learned on the way is kept in the roadmap, as tr_roadmap_solve keeps it.
 *   2. IK from states[N_q[i]] to r_q for every i: ALL n k problems in one tr_ik_batch_dev (x_i, tip_i, err_i: tr_ik_batch's bits).
 *   3. (ok_i, t_i) = checkMotion(states[N_q[i]], x_i, last_valid): tr_validate_edges_last_valid's bits.
 *   4. TR_TIPQ_REACHED: the first i in neighbour order with err_i < tolerance and ok_i (:3214-3287) -> controls x_i, tip_i, err_i,
 *      connection vertex N_q[i], t = 1.
 *   5. TR_TIPQ_CLOSEST: otherwise g_i = interpolate(states[N_q[i]], x_i, t_i), its tip from tr_fk_tips, e_i = |tip(g_i) - r_q|;
 *      the smallest e_i, the first winning a tie (:3445-3521) -> controls g_i, its tip, e_i, N_q[i], t_i.
 *   6. (tr_roadmap_solve_tips) tr_roadmap_solve(s_q, connection vertex): status codes as there; the path is the vertex path
 *      followed by the goal state (`controls`); cost = roadmap cost + state-space distance from the connection vertex to it.
 * The result joins the roadmap through that ONE validated edge, as an RMAP_IK_AUTO_ADD result without ACCURATE does in the reference
 * (:3242-3244, :3276-3287).  Deliberate difference: in the CLOSEST case the reference also connects the new vertex lazily to its
 * connection-strategy neighbours (:3534), so its cost may be smaller.  RMAP_IK_LAZY_ADD and persistent insertion into the graph
 * are not offered; the graph is never edited.
 * RMAP_IK_ACCURATE (the *_connect entry points with k_connect > 0; :3237-3244, :3344-3352, :3471-3478): the vertex IK started from
 * is nearest in TIP space; the straight state-space segment from it to the IK answer is often the one that collides while a
 * state-space neighbour of the answer reaches it.  Rules 1, 2 and 6 stay; with N_q[i] the slot's IK vertex:
 *   3'. C_i = tr_roadmap_nearest_states(x_i, k_connect, max_distance), then N_q[i] as the LAST source when C_i does not hold it
 *       (:3238-3241): at most k_connect + 1 sources per slot.  (ok_ij, t_ij) = checkMotion(states[C_i[j]], x_i, last_valid) for every
 *       source j in that order: all live pairs of the call in ONE tr_validate_edges_last_valid.
 *   4'. TR_TIPQ_REACHED: the first (i, j) in lexicographic order with err_i < tolerance and ok_ij -> controls x_i, tip_i, err_i,
 *       connection vertex C_i[j], t = 1.
 *   5'. TR_TIPQ_CLOSEST: otherwise g_ij = interpolate(states[C_i[j]], x_i, t_ij), its tip from tr_fk_tips, e_ij = |tip(g_ij) - r_q|;
 *       the smallest e_ij, the first in (i, j) order winning a tie (:3452-3521) -> controls g_ij, its tip, e_ij, C_i[j], t_ij.
 * neighbor_vertex is the connection vertex (what rule 6 solves to); ik_vertex is N_q[i] of the chosen slot. */
/* Replaces vertexTipPositionProperty_ (filled by voxelizeVertex :2803-2837 or read from the file): tips n_vertices x 3 (NULL: computed
 * once with tr_fk_tips_dev from the roadmap's states); present_bits (optional): a 0 bit = the vertex has no tip and is never a
 * neighbour.  Uploads the tips and a copy of the states. */
int tr_roadmap_set_tips(tr_roadmap *rm, const double *tips, const uint64_t *present_bits);
/* Rule 1 alone -- replaces the nearest-neighbour structure over tips of roadmapIk (:3120-3160; the shim's full stable_sort per request):
 * vertices n x k (-1 padded), dist2 (optional) n x k (+inf where padded).  Exact, brute force over the tip array (tip_knn). */
int tr_roadmap_nearest_tips(tr_roadmap *rm, const double *requests, int64_t n, int32_t k, int32_t *vertices, double *dist2);
int tr_roadmap_nearest_tips_dev(tr_roadmap *rm, const double *d_requests, int64_t n, int32_t k, int32_t *d_vertices, double *d_dist2);
/* k <= 64; ik: the arguments roadmapIk hands to inverse_kinematics (the shim passes 100, 0.1, 1e-9, 1e-4, tolerance, 1e-6).
 * A NULL tr_tip_query_params* means k = 5, tolerance = 1e-4 and those; a NULL tr_space_params* the defaults of Problem.h:59-62. */
typedef struct {
  int32_t k;
  double tolerance;
  tr_ik_params ik;
} tr_tip_query_params;
#define TR_TIPQ_REACHED     0
#define TR_TIPQ_CLOSEST     1
#define TR_TIPQ_NO_NEIGHBOR 2   /* no vertex to start from (roadmapIk returns nothing); outputs NaN, vertex -1 */
/* Rules 1 - 5 -- replaces roadmapIk called once per request (:3095-3577).  Outputs (each may be NULL): controls n x S, tips n x 3,
 * error n, neighbor_vertex n, outcome n (TR_TIPQ_*), last_valid_t n. */
int tr_roadmap_ik_batch(tr_roadmap *rm, const tr_space_params *sp, const tr_tip_query_params *params, const double *requests, int64_t n,
                        double *controls, double *tips, double *error, int32_t *neighbor_vertex, int32_t *outcome, double *last_valid_t);
/* Rules 1 - 6 -- replaces the app's roadmapIk + solveWithRoadmap per waypoint (apps/roadmap_chained_plan.cpp:535-679).  status / cost /
 * path_offsets / stats as tr_roadmap_solve; a request without a neighbour ends TR_QUERY_INVALID_GOAL.  The vertex paths come through
 * tr_roadmap_fetch_paths as after tr_roadmap_solve; the goal state that follows the last vertex is in `controls`. */
int tr_roadmap_solve_tips(tr_roadmap *rm, const tr_space_params *sp, const tr_tip_query_params *params, const int32_t *starts,
                          const double *requests, int64_t n, int32_t n_threads, double *controls, double *tips, double *error,
                          int32_t *neighbor_vertex, int32_t *outcome, double *last_valid_t, int32_t *status, double *cost,
                          int64_t *path_offsets, tr_roadmap_stats *stats);
/* Host wall time of the phases of the last tr_roadmap_ik_batch / tr_roadmap_solve_tips in milliseconds (instrumentation): out[0] nearest
 * (validity + tip_knn + gather), out[1] IK, out[2] edges, out[3] select (interpolation, FK, choice, results), out[4] solve;
 * out[5] = rounds of the IK batch. */
int tr_roadmap_tip_query_profile(tr_roadmap *rm, double out[6]);
/* The k nearest roadmap vertices of ARBITRARY states (tr_knn answers only for rows of its own array) -- connectionStrategy_(vertex)
 * for a state that is not in the roadmap: queries n x state_size; per query the first k vertices in the order (dist, vertex index)
 * among the vertices valid in the current grid (validity learned and kept as rule 1 does; having a tip is not required); vertices
 * n x k (-1 padded), dist (optional) n x k (+inf where padded).  Entries farther than max_distance are dropped (INFINITY: no bound).
 * dist = CompoundStateSpace::distance in tr_knn's arithmetic, fp64 without contraction: s2 = 0, s2 += t t over the tension
 * differences left to right, sqrt(s2), + w_rot arc (arc = |dtheta|, 2 pi - |dtheta| beyond pi), + w_ret sqrt(ds ds)
 * (tr_space_weights); candidates whose distances round equal stay in index order.  k: 1 .. 64; needs tr_roadmap_set_tips (it uploads
 * the states).  Exact, brute force over the vertex array (state_knn).  The _dev form takes device pointers on the context's GPU and
 * synchronises as tr_roadmap_nearest_tips_dev does: the device before, the null stream after. */
int tr_roadmap_nearest_states(tr_roadmap *rm, const double *queries, int64_t n, int32_t k, double max_distance, int32_t *vertices, double *dist);
int tr_roadmap_nearest_states_dev(tr_roadmap *rm, const double *d_queries, int64_t n, int32_t k, double max_distance, int32_t *d_vertices,
                                  double *d_dist);
/* The accurate rule (3' - 5' above).  k_connect: 0 .. 64; 0, or a NULL tr_tip_connect_params*, is the one-edge rule with its bits and
 * ik_vertex = neighbor_vertex.  n k (k_connect + 1) <= 2^28.  max_distance bounds the source search (INFINITY: none). */
typedef struct {
  int32_t k_connect;
  double max_distance;
} tr_tip_connect_params;
int tr_roadmap_ik_batch_connect(tr_roadmap *rm, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                                const double *requests, int64_t n, double *controls, double *tips, double *error, int32_t *neighbor_vertex,
                                int32_t *ik_vertex, int32_t *outcome, double *last_valid_t);
int tr_roadmap_solve_tips_connect(tr_roadmap *rm, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                                  const int32_t *starts, const double *requests, int64_t n, int32_t n_threads, double *controls, double *tips,
                                  double *error, int32_t *neighbor_vertex, int32_t *ik_vertex, int32_t *outcome, double *last_valid_t,
                                  int32_t *status, double *cost, int64_t *path_offsets, tr_roadmap_stats *stats);
/* Of the last *_connect call on this roadmap: out[0] pairs checked, out[1] requests REACHED, out[2] requests whose connection vertex
 * differs from their ik_vertex, out[3] requests REACHED that the one-edge rule, restricted to the pairs (i, N_q[i]), does not reach.
 * The source search counts into `nearest` of tr_roadmap_tip_query_profile. */
int tr_roadmap_tip_connect_stats(tr_roadmap *rm, int64_t out[4]);

/* ---- queries between ARBITRARY states: attach on the device, seeded search ----------------------------------
 * tr_roadmap_solve answers for pairs of roadmap VERTICES.  The reference's solvePrep (motion-planning/VoxelCachedLazyPRM.cpp:2978-3020)
 * turns the problem's start and goal STATES into milestones with addMilestone(state, connect = true) (:1854-1885), which joins each to
 * its connectionStrategy_ neighbours, and A* runs over the augmented graph; apps/roadmap_chained_plan.cpp:533,548-552 starts every hop
 * at the state the robot is in.  Here that is two primitives and their composition; the graph itself is never edited.
 *
 * Attach (tr_roadmap_attach_states): for n states (n x state_size; any state of the space, retraction and rotation robots included)
 * and a direction -- TR_ATTACH_OUT: the motion LEAVES the state, TR_ATTACH_IN: it ARRIVES at it --
 *   A1. valid[i] (one byte) is tr_validate_batch's bit for the state under the installed checker and the current grid (solvePrep only
 *       admits valid states).
 *   A2. vertices[i][0..k) and cost[i][0..k) are exactly tr_roadmap_nearest_states(state_i, k, max_distance): the (dist, vertex index)
 *       order among the vertices valid in the current grid, tr_knn's arithmetic, -1 / +inf padding; the vertex validity learned on the
 *       way is kept in the roadmap.  An INVALID state gets a row of -1 / +inf.
 *   A3. edge_ok[i][j] (one byte) is the verdict bit of checkMotion(state_i, states[vertices[i][j]]) for OUT, of
 *       checkMotion(states[vertices[i][j]], state_i) for IN: the bit tr_validate_edges gives for the pair in that order.  Padded slots
 *       and the slots of invalid states give 0 and take no FK sample.
 *   A4. n_fk (optional, n x k) are the FK samples per slot as tr_validate_edges_indexed counts them over the array [roadmap states |
 *       query states] (end states once per array, not per pair); n_domain_errors (optional) as in the edge calls.
 * A state's row does not depend on the other states, their order or n.  k: 1 .. 64; a NULL tr_attach_params* means k = 10 and INFINITY
 * (connect_k's defaults); a NULL tr_space_params* the defaults of Problem.h:59-62.  Needs tr_roadmap_set_tips, as
 * tr_roadmap_nearest_states does; n == 0: TR_OK.  Between the states going up and the result arrays coming down the index PAIRS never
 * cross the bus, only their number: tr_validate_batch_dev -> state_knn -> the live slots compacted in slot order into index pairs
 * over one device array (the roadmap's rows, resident from the first call on, with the query rows behind them; attach_kernel.hpp) ->
 * ONE tr_validate_edges_indexed_dev -> the verdict words scattered back to n x k bytes.  What that edge call computes does pass
 * through the host INSIDE it, as in every use of it: its per-pair results come down, and the packed verdict words (one bit per pair;
 * with n_fk also the counts, 4 bytes per pair) go up again to the arrays the scatter reads.  The _dev form takes and returns device pointers
 * on the context's GPU with the same bits and synchronises as tr_roadmap_nearest_states_dev does. */
#define TR_ATTACH_OUT 0
#define TR_ATTACH_IN  1
typedef struct {
  int32_t k;
  double max_distance;
} tr_attach_params;
int tr_roadmap_attach_states(tr_roadmap *rm, const tr_space_params *sp, const tr_attach_params *params, int32_t direction,
                             const double *states, int64_t n, uint8_t *valid, int32_t *vertices, double *cost, uint8_t *edge_ok,
                             int32_t *n_fk, int64_t *n_domain_errors);
int tr_roadmap_attach_states_dev(tr_roadmap *rm, const tr_space_params *sp, const tr_attach_params *params, int32_t direction,
                                 const double *d_states, int64_t n, uint8_t *d_valid, int32_t *d_vertices, double *d_cost,
                                 uint8_t *d_edge_ok, int32_t *d_n_fk, int64_t *n_domain_errors);
/* Seeded search -- a search from several weighted sources to several weighted targets (the reference's TODO :2011-2013, "Solve A* with
 * multiple goals simultaneously").  Query q has source seeds (u_i, c_i) = (src_vertices, src_costs)[src_offsets[q] .. src_offsets[q+1])
 * and target seeds (v_j, d_j) likewise; vertices in [0, n_vertices) (else TR_ERR_OUT_OF_RANGE), costs finite and >= 0 (else
 * TR_ERR_INVALID_ARG); direct_cost[q] (optional array; +inf or NULL: none) is the cost of a connection that bypasses the roadmap.
 *   S1. The answer minimises c_i + dist(u_i, v_j) + d_j, dist = the shortest path in the roadmap minus the items invalid in the current
 *       grid; u_i == v_j is allowed (an empty roadmap part).  The direct connection wins when direct_cost <= that minimum.
 *   S2. Validity is found lazily exactly as tr_roadmap_solve finds it: the same rounds of candidate paths, the same K4 launches, the same
 *       three eager rules, TENDON_HIP_LAZY_ONLY honoured; what a call learns is kept for the next.  Seed vertices of unknown validity
 *       are tested before the first search, as the end points of tr_roadmap_solve are; an invalid seed vertex drops its seed.
 *   S3. cost is summed left to right from the source: ((c_i + w_1) + w_2 ...) + d_j, which is A*'s own g.
 *   S4. status: TR_QUERY_SOLVED, or TR_QUERY_NO_PATH -- no finite combination, an empty seed list without a direct cost included.
 *       src_pick / dst_pick (optional): indices into the query's seed lists, -1 when the direct connection won or there is no path;
 *       path_offsets and tr_roadmap_fetch_paths: the vertex path u_i ... v_j, empty for a direct answer; stats as tr_roadmap_solve.
 * A query's answer does not depend on the batch.  The searches (astar_seeded: the sources enter the open list with g = c_i, a virtual
 * goal is relaxed with g(v_j) + d_j when a target vertex is expanded, heuristic min_j (h(v, v_j) + d_j), landmark terms included) run
 * on the HOST THREADS at every batch size: the rounds of this call never launch roadmap_astar, and tr_roadmap_search_stats out[0]
 * stays 0 after it. */
int tr_roadmap_solve_seeded(tr_roadmap *rm, int64_t n_queries, const int64_t *src_offsets, const int32_t *src_vertices,
                            const double *src_costs, const int64_t *dst_offsets, const int32_t *dst_vertices, const double *dst_costs,
                            const double *direct_cost, int32_t n_threads, int32_t *status, double *cost, int32_t *src_pick,
                            int32_t *dst_pick, int64_t *path_offsets, tr_roadmap_stats *stats);
/* State-to-state queries -- solvePrep + solveWithRoadmap for n (start state, goal state) pairs (starts, goals: n x state_size).  ONE
 * attach pass: the starts attached OUT, the goals IN, and the direct edges checkMotion(start_q, goal_q) where the rule below applies,
 * the pairs of all three in one edge-check call.  Then:
 *   T1. an invalid start state: TR_QUERY_INVALID_START; otherwise an invalid goal state: TR_QUERY_INVALID_GOAL (solvePrep :2995-3010).
 *   T2. the direct edge is tried when both states are valid and d(start, goal) <= max(cost_s[k-1], cost_g[k-1]) (padding counts as
 *       +inf) and <= max_distance: when the other state would be among the k nearest if it were a milestone, as in the reference after
 *       both addMilestone calls.  d in tr_knn's arithmetic.
 *   T3. otherwise the result of the seeded search: seeds = the slots with edge_ok, at their attach distances; direct_cost =
 *       d(start, goal) when the direct edge is valid.
 * Outputs (status and path_offsets required, the others may be NULL): cost; start_vertex / goal_vertex, the picked connection
 * vertices (-1 for a direct answer or none); direct (one byte); src_pick / dst_pick, the picked SLOTS of the attach rows (0 .. k-1,
 * -1 likewise); the vertex paths through tr_roadmap_fetch_paths (start state and goal state precede and follow them).
 * Deliberate differences from the reference: nothing is inserted into the graph; the attachments are validated eagerly in one batch
 * instead of lazily; the neighbours are drawn from the vertices valid in the current grid. */
int tr_roadmap_solve_states(tr_roadmap *rm, const tr_space_params *sp, const tr_attach_params *params, const double *starts,
                            const double *goals, int64_t n, int32_t n_threads, int32_t *status, double *cost, int32_t *start_vertex,
                            int32_t *goal_vertex, uint8_t *direct, int32_t *src_pick, int32_t *dst_pick, int64_t *path_offsets,
                            tr_roadmap_stats *stats);
/* Host wall time of the phases of the last tr_roadmap_solve_states in milliseconds (instrumentation): out[0] validity + nearest +
 * pairs, out[1] edges, out[2] seeded search, out[3] results. */
int tr_roadmap_state_query_profile(tr_roadmap *rm, double out[4]);

/* ---- tip-goal queries on LOADED shapes ----
 * With TendonRobot::general_shape installed as the checker's FK (apps/profile_chained_plan.cpp:407-451) roadmapIk takes every shape
 * from voxelStateChecker_->fk (:3052, :3187): its IK, its last-valid edge checks and its closest-state rule all run on loaded shapes.
 * These calls are that for ONE load set per call (`loads`: tr_edge_loads' meaning of BASE and WORLD, NULL: no load; warm_start is not
 * read -- every solve is cold).  `shoot` goes to all three solvers (NULL: each one's own defaults -- tr_ik_loaded_batch's for the IK,
 * tr_fk_loaded_batch's for the pair check and rule 5L).  `connect` NULL or k_connect 0: the one-edge rule.  Rules 1 - 6 with:
 *   1L.  Rule 1 unchanged.  The tips are the roadmap's and must be LOADED tips: given to tr_roadmap_set_tips by the caller, or made by
 *        tr_roadmap_set_tips_loaded.  Tips the roadmap computed itself with tr_fk_tips_dev (the NULL form of tr_roadmap_set_tips) are
 *        unloaded ones: TR_ERR_INVALID_ARG.
 *   2L.  ALL n k problems in ONE tr_ik_loaded_batch_dev, cold (guess = NULL), bounds as in rule 2: x_i, tip_i, err_i, vu0_i,
 *        equilibrium_i -- that call's bits.
 *   3L / 3'L.  (ok, t) = checkMotion(source, x_i, last_valid) on loaded samples: all live pairs of the call in ONE
 *        tr_validate_edges_loaded with last_valid_t, the same loads, cold.  A sample that does not converge is an invalid sample.
 *        (Host-array form, as the unloaded rule's.)
 *   4L / 4'L.  TR_TIPQ_REACHED additionally needs equilibrium_i.
 *   5L / 5'L.  The tip of g = interpolate(source, x_i, t) comes from a cold tr_fk_loaded_tips_dev solve of g under g's own load rows
 *        (WORLD loads turned by g's rotation: edge_sincos, the rows of the pair check's samples), one solve per live pair.  A g whose
 *        solve does not converge is not a candidate.  A request with a neighbour but no candidate ends TR_TIPQ_NO_NEIGHBOR (outputs
 *        NaN, vertices -1): a state without an equilibrium is never handed out as a goal.
 *   6.   Rule 6 unchanged (the cached sets of a roadmap built under loads are loaded sets already).
 *   vu0 (optional, n x 6): the base strains of the chosen state -- the IK's when REACHED, the g solve's when CLOSEST, NaN otherwise.
 *   counts (optional, int64[4]): pairs checked, IK answers without an equilibrium (slots that hold a neighbour), g solves
 *        unconverged, integrations (the IK's of those slots + the pair check's + the g solves').
 * Every result row is a function of its request, the roadmap, the grid, the loads and the parameters alone: not of the rest of the
 * batch, not of TENDON_HIP_SHOOT_CHUNK.  tr_roadmap_tip_query_profile and tr_roadmap_tip_connect_stats answer for these calls too.
 * Robots with retraction: TR_ERR_UNSUPPORTED; a bad frame or max_iters < 0: TR_ERR_INVALID_ARG; n == 0: TR_OK before anything else
 * is asked for.  The calls run on the null stream and share the context's one shooting workspace. */
int tr_roadmap_ik_batch_loaded(tr_roadmap *rm, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                               const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *requests, int64_t n, double *controls,
                               double *tips, double *error, int32_t *neighbor_vertex, int32_t *ik_vertex, int32_t *outcome,
                               double *last_valid_t, double *vu0, int64_t *counts);
int tr_roadmap_solve_tips_loaded(tr_roadmap *rm, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                                 const tr_shoot_params *shoot, const tr_edge_loads *loads, const int32_t *starts, const double *requests, int64_t n,
                                 int32_t n_threads, double *controls, double *tips, double *error, int32_t *neighbor_vertex, int32_t *ik_vertex,
                                 int32_t *outcome, double *last_valid_t, double *vu0, int64_t *counts, int32_t *status, double *cost,
                                 int64_t *path_offsets, tr_roadmap_stats *stats);
/* tr_roadmap_set_tips with the tips of the vertices' LOADED shapes: one cold tr_fk_loaded_tips_dev solve per vertex under its own load
 * rows.  A vertex whose solve does not converge has no tip (its present bit is cleared). */
int tr_roadmap_set_tips_loaded(tr_roadmap *rm, const tr_shoot_params *shoot, const tr_edge_loads *loads, const uint64_t *present_bits);

/* The connection loop itself (motion-planning/VoxelCachedLazyPRM.cpp:1491-1502: for every vertex v and every neighbour n
 * of connectionStrategy_(v), `if (!getEdge(v, n)) connectVertices(v, n)`): the undirected edge set of the k-nearest
 * table -- pairs (lo, hi), lo < hi, each once, ordered by (lo, hi) -- built on the device (sort + unique of the pair
 * keys); only the edge list crosses PCIe.  k counts the vertex itself, as in tr_knn.  edges: capacity x 2 int32; *n_edges
 * receives the number of edges (if it exceeds capacity only the first `capacity` are written: at most n (k - 1) edges exist -- n k when k or more states coincide, a row then need not hold its own vertex). */
int tr_knn_edges(tr_ctx *ctx, const double *states, int64_t n, int32_t k, double max_distance, int32_t *edges,
                 int64_t capacity, int64_t *n_edges);
/* Device-resident form of the connection loop and of the edge checks after it: d_states (n x state_size doubles) and d_edges
 * (capacity x 2 int32) are device arrays on the context's GPU, so a roadmap whose vertices were produced there (sampled or
 * filtered on the device) is connected and validated without its states or its edge list crossing PCIe -- only *n_edges, and
 * from tr_validate_edges_indexed_dev the mask words (d_valid_bits: (n_edges + 63) / 64 words; d_n_fk: n_edges counts or NULL),
 * which are device arrays too.  Same results, order and error codes as tr_knn_edges / tr_validate_edges_indexed; both calls
 * synchronise with the device on entry (the inputs may have been written on any stream) and before they return.
 * Where the host form falls back to gathering the end states on the host (more vertices than half the sample pool: beyond 2^23
 * vertices, or under a bounded pool) tr_validate_edges_indexed_dev brings its inputs over and does the same: correct, not fast. */
int tr_knn_edges_dev(tr_ctx *ctx, const double *d_states, int64_t n, int32_t k, double max_distance, int32_t *d_edges,
                     int64_t capacity, int64_t *n_edges);
int tr_validate_edges_indexed_dev(tr_ctx *ctx, const tr_space_params *sp, const double *d_states, int64_t n_states,
                                  const int32_t *d_edges, int64_t n_edges, uint64_t *d_valid_bits, int32_t *d_n_fk,
                                  int64_t *n_domain_errors);
/* Vertices that have just passed the vertex phase need not be integrated again by the edge call (every indexed edge call otherwise
 * evaluates each vertex once for its signature: 1.4 ms per 10^5 vertices, and the same on every rank when the edge list is sharded):
 * tr_validate_candidates_sig_dev is tr_validate_candidates_dev that also writes each candidate's backbone cell signature, a row of
 * tr_signature_words(ctx) uint32 (an even number; meaningful where the candidate's bit is set); compact the rows of the accepted
 * candidates like their states (tr_compact_rows_dev with row_doubles = tr_signature_words / 2) and pass them as d_vertex_sig
 * (n_states rows) to tr_validate_edges_indexed_sig_dev, which then treats every vertex as valid and gives the verdicts, counts and
 * errors of tr_validate_edges_indexed_dev.  tr_signature_words returns 0 -- and the two calls TR_ERR_UNSUPPORTED -- for retraction
 * robots, under TR_CHECKER_SPHERES and on schedules other than the default verdict-only one. */
int tr_signature_words(const tr_ctx *ctx);
/* ... and tr_sample_valid_vertices_dev that also returns the accepted vertices' rows (d_sig: n_want x tr_signature_words uint32, row i
 * belongs to d_states row i): createRoadmap's "sample until N are valid" feeding the edge phase directly. */
int tr_sample_valid_vertices_sig_dev(tr_ctx *ctx, uint64_t seed, uint64_t first_candidate, const double *lo, const double *hi,
                                     int64_t n_want, int64_t max_candidates, double *d_states, double *d_tips, int64_t *d_index,
                                     uint32_t *d_sig, int64_t *n_accepted, int64_t *n_tried, void *stream);
int tr_validate_candidates_sig_dev(tr_ctx *ctx, uint64_t seed, uint64_t first, int64_t count, const double *lo, const double *hi,
                                   uint64_t *d_valid_bits, double *d_tips, uint32_t *d_sig, void *stream);
int tr_validate_edges_indexed_sig_dev(tr_ctx *ctx, const tr_space_params *sp, const double *d_states, int64_t n_states,
                                      const uint32_t *d_vertex_sig, const int32_t *d_edges, int64_t n_edges,
                                      uint64_t *d_valid_bits, int32_t *d_n_fk, int64_t *n_domain_errors);

/* The signature rows on the wire.  They are the one large collective of a sharded roadmap build (576 B per vertex at 129 backbone
 * points: 346 MB per build of 6 x 10^5 vertices), and they are redundant: consecutive backbone points lie at most dL <= one voxel edge
 * apart (the checker's constructor enforces it), so consecutive cells of a row differ by -1, 0 or +1 per axis.  A packed row =
 * the first point's word, then 6 bits per further point, padded to tr_signature_packed_words(ctx) uint32 (an even number: 26 = 104 B
 * at 129 points).  tr_pack_signatures_dev packs n_rows rows (d_sig: n_rows x tr_signature_words) and reports in *n_uncodable the rows
 * it could not code (a point outside the voxel domain, or a larger step: never for vertices that passed the vertex phase) -- the
 * caller then sends the rows as they are; it synchronises `stream` (one counter read-back).  tr_unpack_signatures_dev restores the rows
 * word for word (the padding words of a row beyond the backbone's points come back as zeros; nothing reads them). */
int tr_signature_packed_words(const tr_ctx *ctx);
int tr_pack_signatures_dev(tr_ctx *ctx, const uint32_t *d_sig, int64_t n_rows, uint32_t *d_packed, int64_t *n_uncodable, void *stream);
int tr_unpack_signatures_dev(tr_ctx *ctx, const uint32_t *d_packed, int64_t n_rows, uint32_t *d_sig, void *stream);

/* The same neighbour lists for a RANGE of the states as queries (all n states remain the candidates): rows
 * first_query .. first_query + n_queries - 1 of tr_knn's tables, whatever the range -- one rank's share when the connection
 * loop of a large roadmap is spread over several GPUs.  idx / dist: n_queries x k. */
int tr_knn_range(tr_ctx *ctx, const double *states, int64_t n, int64_t first_query, int64_t n_queries, int32_t k,
                 double max_distance, int32_t *idx, double *dist);
/* The undirected edge set of a k-nearest table given by the caller (n x k indices, -1 = none; e.g. the ranks' tr_knn_range
 * rows gathered): what tr_knn_edges builds from its own table, with the same order and capacity rule. */
int tr_knn_table_edges(tr_ctx *ctx, const int32_t *idx, int64_t n, int32_t k, int32_t *edges, int64_t capacity, int64_t *n_edges);
/* Device-resident forms of the two calls above, for the sharded connection loop of a roadmap whose vertices are in HBM: the rank's rows
 * go to a device array (all-gathered there), the gathered table's edge list is written straight into d_edges.  Same rows, edges,
 * order and error codes; both synchronise with the device on entry and before they return. */
int tr_knn_range_dev(tr_ctx *ctx, const double *d_states, int64_t n, int64_t first_query, int64_t n_queries, int32_t k,
                     double max_distance, int32_t *d_idx);
int tr_knn_table_edges_dev(tr_ctx *ctx, const int32_t *d_idx, int64_t n, int32_t k, int32_t *d_edges, int64_t capacity,
                           int64_t *n_edges);

/* k of the PRM* connection strategy for a roadmap of n_milestones vertices (og::KStarStrategy as installed by
 * setStarConnectionStrategy, motion-planning/VoxelCachedLazyPRM.cpp:1346-1356): ceil((e + e / dim) * ln(n)), dim =
 * state dimension.  createRoadmap connects after all vertices are in place, so this k applies to every vertex of the
 * batch: pass k + 1 to tr_knn (row i holds i itself first).  -1 on bad arguments. */
int tr_kstar_k(const tr_ctx *ctx, int64_t n_milestones);

/* ---- instrumentation ---------------------------------------------------------------------- */

/* Time the last `which` kernel launches with HIP events on the stream they ran on.
 * tr_profile_begin enables event recording around every kernel launched by this context;
 * tr_profile_read returns, per kernel slot, launches and total milliseconds since begin.
 * slots: 0 = fk_rk4_batch, 1 = backbone_voxel_sweep, 2 = cached_blocks_vs_grid, 3 = edge helpers,
 * 4 = fk_sweep_fused (K1 + K2 in one launch over stored points: edge samples, voxel caches, the sphere checker, and the
 *     fallback pass of the verdict path), 5 = fk_verdict (the verdict-only kernel of tr_validate_batch* and of the edge
 *     samples; fk_verdict_retract for retraction-enabled robots -- the ordering of its batch by backbone length runs
 *     outside the slot) */
#define TR_PROFILE_SLOTS 6
int tr_profile_begin(tr_ctx *ctx);
int tr_profile_read(tr_ctx *ctx, int64_t launches[TR_PROFILE_SLOTS], double total_ms[TR_PROFILE_SLOTS]);
int tr_profile_end(tr_ctx *ctx);

/* debug / A-B switches (tests): bit0 = brute-force O(P^2) self-collision instead of the
 * conservative-skip sweep (verdicts must be identical); bit1 = no milestone proof of "no self collision": every
 * configuration takes the exact pairwise sweep (the fallback pass of the verdict path, the in-wave sweep of the edge queue);
 * bit2 = no dilated-grid fast path in the voxel walk.  Verdicts, flags and FK counts are the same under every combination. */
int tr_set_debug(tr_ctx *ctx, uint32_t bits);

/* How the last tr_validate_edges_indexed* call of this context was scheduled (instrumentation; tests assert on it):
 *   stats[0]  FK samples the edge queue took (0: the call ran on the level-synchronous lanes)
 *   stats[1]  rounds: batches of up to 64 samples a persistent wave integrated
 *   stats[2]  samples whose self-collision test took the exact pairwise sweep inside the queue
 *   stats[3]  flags the queue ended with: 0 = complete; 1 = sample pool too small, 4 = an edge level of more than 2048 intervals
 *             (in both cases the lanes then took the call); 2 = a wait made no progress (the call returned TR_ERR_RUNTIME)
 * The edge queue (csrc/edge_queue_kernel.hpp) is ONE persistent launch over a device work queue with a barrier per edge instead of
 * one per level of all edges: same verdicts, FK counts and domain-error count as the lanes, bit for bit. */
int tr_edge_schedule_last(const tr_ctx *ctx, uint32_t stats[4]);

/* Environment switches, read ONCE by tr_create (a context keeps what it read).  They exist for A/B measurements and for
 * tests that must reach a rarely taken path; none of them changes a result, and production code sets none of them.
 *   TENDON_HIP_FUSED=0|1|2          schedule of tr_validate_batch*: 2 (default) verdict-only kernel, 1 K1 + K2 as one kernel over
 *                                   stored points, 0 separate launches (the edge queue, the signature hand-over and
 *                                   tr_sample_valid_vertices* need 2 and report TR_ERR_UNSUPPORTED or fall back otherwise)
 *   TENDON_HIP_EDGE_QUEUE=0|1       unset: the device-resident indexed edge checks (tr_validate_edges_indexed_dev / _sig_dev) go through
 *                                   the edge queue where it applies (no retraction, schedule 2), the host-array form through the
 *                                   level-synchronous lanes; 1: both through the queue; 0: both through the lanes
 *   TENDON_HIP_EDGE_QUEUE_WAVES=n   persistent workgroups of the edge queue (default: what the device holds at once)
 *   TENDON_HIP_EDGE_LANES=1..4      exactly that many lanes of the level-synchronous edge bisection (default: by the edge count)
 *   TENDON_HIP_EDGE_LANE_GUESS=x    samples per edge assumed when a lane is given its share of the pool (tests: a small value
 *                                   provokes the overflow path)
 *   TENDON_HIP_EDGE_POOL=n          upper bound of the FK sample pool (tests: forces chunking / the overflow paths)
 *   TENDON_HIP_FB_CAP=n             columns of the fallback pass's point workspace (default: one resident round of waves)
 *   TENDON_HIP_SHOOT_CHUNK=n        problems per chunk of tr_fk_loaded_batch* (tests: forces chunking; default: what 2^19 lanes hold)
 *   TENDON_HIP_LOADED_VERTEX_BATCH=n  candidates per batch of tr_sample_valid_vertices_loaded* and states per chunk of
 *                                   tr_voxelize_batch_loaded (tests: several batches; default: 2^16, what the workspace is grown to)
 *   TENDON_HIP_RETRACT_SORT=n       retraction robots: batches of at least n configurations are ordered by backbone length
 *                                   (0 = never); TENDON_HIP_RETRACT_KBEGIN_OFF: no per-wave loop start in that order
 *   TENDON_HIP_LOADED_RETRACT_SORT=n  retraction robots: a shooting run (tr_loaded_order_last) of at least n problems is solved in
 *                                   backbone-length order (0 = never); the results are the bits of the arrival-order solve
 *   TENDON_HIP_ROUTING=table        the general (table) form of the strain right-hand side for every robot.  Unset: a robot without
 *                                   retraction whose tendons all have constant radius and at most linear angle, with ONE pitch and
 *                                   ONE radius (compared bit for bit; straight tendons: pitch 0), of at most six tendons, gets the
 *                                   uniform-helix form in every unloaded shared-grid kernel (csrc/fk_kernel.hpp: UniformHelix): the
 *                                   same quantities from fewer instructions, equal to the table form's up to the rounding of the
 *                                   last bits (both within the bound of tests/test_gpu_fk_truth.py)
 * Read per call (the tests switch between two paths inside one process; the switches of tr_roadmap_*: once, at the start of the call
 * that uses them -- csrc/roadmap.hip: read_switches):
 *   TENDON_HIP_KNN=lanes            neighbour search by the lane-per-query kernel for every k (default: wave per query up to k = 64);
 *                                   TENDON_HIP_KNN_CELL=x scales its cell width (tuning)
 *   TENDON_HIP_MERGE=sort           edge voxel sets merged by the segmented sort (default: the per-edge LDS table);
 *                                   TENDON_HIP_MERGE_MAXLOAD=n bounds that table's load (tests: reaches the overflow fallback)
 *   TENDON_HIP_LANDMARKS=...        landmark choice of tr_roadmap_prepare (csrc/roadmap.hip; tuning)
 *   TENDON_HIP_SEARCH=host|device   graph searches of tr_roadmap_solve: unset = a round of 512 or more queries is shared between the
 *                                   roadmap_astar kernel and the host threads (below), a smaller round is the host threads'; host =
 *                                   the host threads always; device = the kernel always, whole rounds, no budget (tests)
 *   TENDON_HIP_SEARCH_HOST_SHARE=p  per cent of a shared round's searches (the ones with the most distant end points) that the host
 *                                   threads take while the kernel runs (default: starts at 1 and follows the two sides' times per roadmap)
 *   TENDON_HIP_SEARCH_BUDGET=n      expansions after which the kernel hands a search back: the host threads start on it at once, while
 *                                   the kernel is still running (a word per query in pinned memory tells them) (default: starts at 6500,
 *                                   or a sixteenth of the roadmap's vertices if that is more, and doubles per roadmap while more than
 *                                   one search in fifty comes back; 0 none)
 *   TENDON_HIP_SEARCH_K=1..12       vertices the kernel takes off a search's open list per step, at most (default 12: as many as their
 *                                   arcs fill the 64 lanes of the step's two passes; 1 = the host's order)
 *   TENDON_HIP_SEARCH_SWEEP=n       expansions after which a host search is handed to the device sweep (tr_roadmap_search_sweeps; 0 never)
 *   TENDON_HIP_SEARCH_SLOTS=n       searches in flight on the device, at most (default: what it holds: 12 waves per CU; a round of
 *                                   fewer queries allocates tables for that many only)
 *   TENDON_HIP_SEARCH_LC0=8..14     log2 of the per-vertex records a search in flight owns (default 12: 176 KiB per slot with its far list;
 *                                   the searches' state does not depend on the roadmap's size); TENDON_HIP_SEARCH_POOL=a,b,c: shared tables of
 *                                   4 / 16 / 64 times that size for the searches that outgrow it (default slots, slots / 4, slots / 64: 5.3 GB in all at 3 072 slots; a search
 *                                   that finds none free is handed back to the host threads).  Both read when a roadmap's first large
 *                                   round sets the searches up (tests reach the growth and hand-back paths with small values)
 *   TENDON_HIP_LAZY_ONLY=1          tr_roadmap_solve never looks at items off the candidate paths (default: when at least
 *                                   max(4, cached sets / 2^17) queries are still open after a round -- or a round's candidate paths hold a
 *                                   quarter as many items as there are cached sets, or the batch has a 256th as many queries as there
 *                                   are cached sets to begin with --, every cached set is tested in one
 *                                   launch and the next round is the last; same answers; the rules read counts, not clocks, so
 *                                   rounds / items_checked / the validity left behind are reproducible; `expanded` depends on which
 *                                   side -- kernel or host threads -- ran a search)
 *   TENDON_HIP_COMPONENTS=0|1       component labels of the roadmap minus the invalid items (queries across components are answered "no
 *                                   path" without a search): unset = from the moment they would have paid on this roadmap (a search
 *                                   walked 2000 vertices in vain, or the kernel handed searches back), 1 = every round of 64 queries
 *                                   or more, 0 = never (a query with an unreachable goal is searched to exhaustion)
 *   TENDON_HIP_PIPE_LOG2=n          chunk size 2^n of tr_validate_batch's host-buffer pipeline (tuning)
 * Output on stderr only: TENDON_HIP_EDGE_TIMING, TENDON_HIP_VOX_TIMING, TENDON_HIP_ROADMAP_TIMING, TENDON_HIP_SEARCH_STATS (where a
 * round's searches ran and for how long), TENDON_HIP_SEARCH_HIST (expansions per search, host searches only). */

#ifdef __cplusplus
}
#endif
#endif /* TENDON_HIP_H */
