/*
 * tgsim.h -- C-ABI of libtgsim.so, the MI355X-native articulated-body
 * simulator that replaces the IsaacGym/PhysX tensor API as the reference task
 * code uses it.  Plain C types only (device pointers are passed as raw
 * pointers, sizes as ints); no torch or HIP types appear in any signature.
 *
 * Reference interface each entry point replaces (paths relative to
 * /root/reference/isaacgymenvs/):
 *
 *   tg_sim_create            gym.create_sim + load_asset + create_env/actor loop
 *                            + prepare_sim   (tasks/base/vec_task.py:51-57,217;
 *                            tasks/gogoro_new.py:155-162,196-294)
 *   tg_sim_destroy           (process teardown)
 *   tg_state_ptrs            acquire_actor_root_state_tensor /
 *                            acquire_dof_state_tensor + gymtorch.wrap_tensor
 *                            (tasks/gogoro_new.py:125-130)
 *   tg_refresh               refresh_actor_root_state_tensor /
 *                            refresh_dof_state_tensor (gogoro_new.py:141-142,426-427)
 *                            -- the views are the live state, nothing is copied; it
 *                            is REQUIRED after writes through the dof_props /
 *                            env_dirty views (it re-arms the compose launch the
 *                            library otherwise skips while no env can be dirty)
 *   tg_set_dof_position_targets / tg_set_dof_velocity_targets
 *                            set_dof_position_target_tensor /
 *                            set_dof_velocity_target_tensor (gogoro_new.py:364,369)
 *   tg_set_actor_root_state_indexed
 *                            set_actor_root_state_tensor_indexed (gogoro_new.py:547)
 *   tg_set_dof_state_indexed set_dof_state_tensor_indexed (gogoro_new.py:552)
 *   tg_set_dof_properties_indexed
 *                            set_actor_dof_properties per env (gogoro_new.py:294,601)
 *   tg_set_body_mass_scale_indexed / tg_set_gravity
 *                            rigid_body_properties.mass / sim_params.gravity
 *                            domain randomisation (vec_task.py:538-768)
 *   tg_set_shape_friction_indexed
 *                            set_actor_rigid_shape_properties (gogoro_new.py:284-293)
 *   tg_apply_rigid_body_force_tensors
 *                            apply_rigid_body_force_tensors(sim, forces [N*L,3],
 *                            torques [N*L,3] | None, space)
 *                            (tasks/gogoro_realistic_turning_sim_paper.py:457)
 *   tg_apply_body_forces     the same, pre-reduced: one wrench per group [N,G,6]
 *   tg_simulate              gym.simulate (vec_task.py:335): sim.substeps substeps
 *   tg_set_net_contact_force_tensor
 *                            acquire_net_contact_force_tensor /
 *                            refresh_net_contact_force_tensor
 *                            (tasks/anymal.py:113,117)
 *   tg_set_dof_force_tensor  acquire_dof_force_tensor / refresh_dof_force_tensor
 *                            (tasks/MA_OP3.py:91,96), with
 *                            enable_actor_dof_force_sensors (:275) implied
 *   tg_set_force_sensor_tensor
 *                            acquire_force_sensor_tensor /
 *                            refresh_force_sensor_tensor, with
 *                            create_asset_force_sensor implied
 *                            (tasks/humanoid.py:80,167-168,243)
 *   tg_jacobians             acquire_jacobian_tensor / refresh_jacobian_tensors
 *                            (tasks/gogoro/gogoro.py:108-114,396-397,507, the
 *                            rider's hand IK; tasks/franka_cube_stack.py:389-393,
 *                            440-441)
 *   tg_mass_matrices         acquire_mass_matrix_tensor /
 *                            refresh_mass_matrix_tensors
 *                            (tasks/franka_cube_stack.py:393,441,
 *                            operational-space control)
 *   tg_ik_dls                the rider's hand IK, damped least squares on one
 *                            link's Jacobian block added to the position targets
 *                            (tasks/gogoro/gogoro.py:381-427, with
 *                            orientation_error :605-608; the one-block control
 *                            of tasks/franka_cube_stack.py:392,602-628)
 *   tg_osc                   _compute_osc_torques, operational-space control on
 *                            one link's Jacobian block and the chain's block of
 *                            the mass matrix, clamped to the effort limits
 *                            (tasks/franka_cube_stack.py:602-628)
 *   tg_inverse_dynamics      no reference counterpart (its arm is loaded with
 *                            disable_gravity): the bias force h(q, u) -- gravity
 *                            and Coriolis compensation -- and tau = H a + h in the
 *                            coordinates of tg_jacobians / tg_mass_matrices
 *   tg_centroidal            no reference counterpart: the whole-body centre of
 *                            mass and its velocity, the angular momentum about it,
 *                            the centroidal inertia, the centroidal momentum matrix
 *                            A_G with h_G = A_G u and the momentum-rate bias A_G' u,
 *                            in the coordinates of tg_jacobians / tg_mass_matrices
 *   tg_contact_inverse_dynamics
 *                            no reference counterpart: whole-body inverse dynamics
 *                            under contact -- the base wrench of tau = H a + h
 *                            distributed over up to four contact links by least
 *                            squares, the joint torques that are left and the
 *                            predicted contact wrenches
 *   tg_height_scan           measured_heights: get_heights on init_height_points
 *                            with quat_apply_yaw, and the clipped, scaled height
 *                            observation (tasks/anymal_terrain.py:501-536,
 *                            :301-302), about any link frames, on the surface the
 *                            contacts feel or by the reference's cell rule
 *   tg_imu                   the inertial measurement unit the paper task observes
 *                            ("imu" roll, yaw and their rates with an IMU noise
 *                            and offset, tasks/gogoro_realistic_turning_sim_paper.py
 *                            :55-67, :525-531): orientation, projected gravity,
 *                            gyro and accelerometer readings at link frames
 *   tg_ray_cast              (no counterpart) lidar and depth-camera ranges: rays
 *                            cast from link frames against the heightfield
 *                            solid and the z = 0 plane
 *   tg_proximity             (no counterpart) self-collision sensing: signed
 *                            distances between capsules on the robot's own
 *                            links, their witness points and a per-env summary
 *                            (smallest distance, count and penalty under a margin)
 *   tg_contact_qp            (no counterpart) whole-body inverse dynamics with the
 *                            contact forces confined to friction cones and sole
 *                            outlines: vertex forces of up to four rectangular
 *                            patches by a fixed number of ADMM iterations, the
 *                            joint torques that are left and the base wrench the
 *                            ground cannot supply
 *   tg_get_sim_params / tg_set_sim_params
 *                            gym.get_sim_params / set_sim_params (vec_task.py:650-660)
 *   tg_sync                  fetch_results(sim, True) (vec_task.py:339)
 *   tg_last_error            (replaces the reference's bool returns + assert,
 *                            gogoro_new.py:547,552, and quit() on creation
 *                            failure, vec_task.py:291-293)
 *
 * Every call returns 0 on success and a negative code on error; the message
 * is available from tg_last_error() (thread-local).  Calls are asynchronous
 * on the stream given by tg_set_stream(); inputs are caller-owned device
 * pointers read in stream order and never retained.
 */
#ifndef TGSIM_H
#define TGSIM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_OK 0
/* joint limits: damping and implicit stiffness ramp in over this distance past
 * the limit (rad or m), keeping the step continuous at the limit */
#define TG_LIMIT_RAMP 0.01f

/* widest [lower, upper] window a locked DOF may carry (the reference locks
 * with 1e-4, tasks/gogoro_new.py:257-262); wider is reported as TG_ERR_STATE */
#define TG_LOCK_WINDOW_MAX 1e-3f

#define TG_ERR_ARG -1
#define TG_ERR_HIP -2
#define TG_ERR_MODEL -3
#define TG_ERR_STATE -4

#define TG_JOINT_FIXED 0
#define TG_JOINT_REVOLUTE 1
#define TG_JOINT_PRISMATIC 2

#define TG_SHAPE_TORUS 0   /* params: R_major, r_minor; torus axis = shape z */
#define TG_SHAPE_BOX 1     /* params: half extents x,y,z                     */
#define TG_SHAPE_SPHERE 2  /* params: radius                                 */

/* DOF drive modes (gymapi.DOF_MODE_*) */
#define TG_DOF_MODE_NONE 0
#define TG_DOF_MODE_POS 1
#define TG_DOF_MODE_VEL 2
#define TG_DOF_MODE_EFFORT 3

/* per-env DOF property fields for tg_set_dof_properties_indexed */
#define TG_PROP_STIFFNESS 0
#define TG_PROP_DAMPING 1
#define TG_PROP_EFFORT 2
#define TG_PROP_VELOCITY 3
#define TG_PROP_LOWER 4
#define TG_PROP_UPPER 5
#define TG_PROP_DRIVE_MODE 6  /* values passed as float, rounded */
#define TG_PROP_ARMATURE 7
#define TG_NUM_PROPS 8

/* Articulation model, links in depth-first order (parents before children).
 * Link frames follow URDF: a link's frame is its incoming joint frame.
 * A "group" is a group-root link plus all descendants reached through fixed
 * or locked joints (locked = position fixed per env between resets, the
 * reference's limit-locked joints, tasks/gogoro_new.py:257-262,562-572). */
typedef struct tg_model_desc {
    int32_t num_links;
    int32_t num_dofs;
    int32_t num_groups;
    int32_t num_shapes;
    const int32_t *link_parent;   /* [L] parent link, -1 for the root       */
    const int32_t *link_group;    /* [L] group of each link                 */
    const int32_t *link_dof;      /* [L] dof of the incoming joint, -1 fixed */
    const int32_t *link_jtype;    /* [L] TG_JOINT_*                          */
    const float *link_origin;     /* [L,12] incoming joint origin in parent link frame: R row-major (9), p (3) */
    const float *link_axis;       /* [L,3] joint axis in the link frame      */
    const float *link_inertia;    /* [L,10] mass, com xyz, ixx iyy izz ixy ixz iyz (about com, link axes) */
    const int32_t *group_root;    /* [G] root link of each group             */
    const int32_t *group_parent;  /* [G] parent group, -1 for the floating root */
    const int32_t *dof_locked;    /* [D] 1 if the dof is locked              */
    const int32_t *shape_link;    /* [S] */
    const int32_t *shape_kind;    /* [S] TG_SHAPE_* */
    const float *shape_pose;      /* [S,12] R row-major, p in the link frame */
    const float *shape_params;    /* [S,4] */
    const float *shape_friction;  /* [S] */
    uint64_t model_hash;          /* selects the compiled kernel specialisation */
} tg_model_desc;

/* sim_params (cfg/task/<Task>.yaml "sim" + "physx" blocks, vec_task.py:442-490) */
typedef struct tg_sim_params {
    float dt;                     /* control dt (sim.dt)                   */
    int32_t substeps;             /* sim.substeps                          */
    float gravity[3];             /* sim.gravity                           */
    float linear_damping;         /* AssetOptions.linear_damping           */
    float angular_damping;        /* AssetOptions.angular_damping          */
    float max_depenetration_velocity; /* physx.max_depenetration_velocity  */
    float rest_offset;            /* physx.rest_offset                     */
    float contact_margin;         /* speculative contact distance          */
    float ground_friction;        /* PlaneParams.static_friction           */
    float baumgarte;              /* penetration push-out factor per substep */
    float limit_stiffness;        /* implicit limit spring, fraction of joint inertia / h^2 */
    float limit_damping;          /* implicit limit damper, fraction of joint inertia / h   */
    int32_t contact_iterations;   /* projected Gauss-Seidel sweeps per substep, with push-out bias
                                     (physx.num_position_iterations) */
    int32_t velocity_iterations;  /* bias-free sweeps after them (physx.num_velocity_iterations):
                                     the positions integrate the velocity of the biased sweeps,
                                     the stored velocity is the bias-free one */
    int32_t fix_base;             /* AssetOptions.fix_base_link            */
    float env_spacing;            /* create_env spacing (env origins grid) */
    int32_t envs_per_row;
    int32_t solver_type;          /* physx.solver_type: 0 PGS, 1 TGS (IsaacGym's default).  TGS runs
                                     the position iterations as sub-steps of h / contact_iterations:
                                     before each sweep a normal row's target is re-formed from its
                                     separation advanced by the row's accumulated displacement, and
                                     the positions integrate the mean of the sweeps' multipliers */
    float contact_offset;         /* physx.contact_offset (IsaacGym default 0.02): PhysX's pair rule --
                                     a shape point carries a (speculative) normal row only while its
                                     separation is below the pair's contact distance, the shape's plus
                                     the ground plane's offset, 2 x contact_offset (round 6; round 5
                                     used one offset plus the point's free approach); <= 0: every
                                     point speculative (the rounds 1-4 behaviour) */
} tg_sim_params;

/* zero-copy device views (gymtorch.wrap_tensor equivalents) */
typedef struct tg_state_view {
    float *root_state;            /* [N,13] pos(3) quat xyzw(4) linvel(3) angvel(3), world frame */
    float *dof_state;             /* [N*D,2] pos, vel */
    float *dof_pos_target;        /* [N,D] */
    float *dof_vel_target;        /* [N,D] */
    float *dof_actuation;         /* [N,D] effort-mode forces */
    float *dof_props;             /* [TG_NUM_PROPS,N,D] */
    float *body_force;            /* [N,G,6] external wrench per group, world frame (force, torque at group COM) */
    float *env_origin;            /* [N,3] */
    uint8_t *env_dirty;           /* [N] */
    int32_t num_envs, num_dofs, num_groups, num_links;
} tg_state_view;

typedef struct tg_sim tg_sim;

int tg_sim_create(const tg_model_desc *model, const tg_sim_params *params, int32_t num_envs, int32_t device,
                  tg_sim **out);
int tg_sim_destroy(tg_sim *sim);
int tg_set_stream(tg_sim *sim, void *hip_stream);
int tg_state_ptrs(tg_sim *sim, tg_state_view *view);
/* Adopt caller-owned device buffers (e.g. torch tensors) for any non-NULL
 * pointer of `view` (sizes as in tg_state_view); the sim's current contents
 * are copied into them first, so the caller's tensors become the live,
 * zero-copy state (the gymtorch.wrap_tensor contract).  Caller keeps them alive. */
int tg_bind_state(tg_sim *sim, const tg_state_view *view);
int tg_refresh(tg_sim *sim);
int tg_set_dof_position_targets(tg_sim *sim, const float *pos);
int tg_set_dof_velocity_targets(tg_sim *sim, const float *vel);
int tg_set_dof_actuation_forces(tg_sim *sim, const float *effort);
int tg_set_actor_root_state_indexed(tg_sim *sim, const float *root, const int32_t *ids, int32_t n);
int tg_set_dof_state_indexed(tg_sim *sim, const float *dof, const int32_t *ids, int32_t n);
int tg_set_dof_properties_indexed(tg_sim *sim, int32_t field, const float *vals, const int32_t *ids, int32_t n);
int tg_set_body_mass_scale_indexed(tg_sim *sim, const float *scale, const int32_t *ids, int32_t n);
int tg_set_shape_friction_indexed(tg_sim *sim, const float *mu, const int32_t *ids, int32_t n);
int tg_set_gravity(tg_sim *sim, const float *g3);
int tg_apply_body_forces(tg_sim *sim, const float *wrench);
/* apply_rigid_body_force_tensors (gymapi; tasks/gogoro_realistic_turning_sim_paper.py:457):
 * forces [N*L,3] acting at each rigid body's centre of mass and torques
 * [N*L,3], either may be NULL (the reference passes torqueTensor=None), in the
 * world frame (TG_ENV_SPACE, isaacgym's default; envs are translated, not
 * rotated) or each body's own frame (TG_LOCAL_SPACE).  Bodies in model.links
 * order (the order of get_actor_rigid_body_dict).  They act for the next
 * tg_simulate call, as PhysX's applied forces do for one simulate: that call
 * reduces them, from the state it starts from, to the group wrenches
 * tg_apply_body_forces takes (world force, torque about the group centre of
 * mass) -- so, unlike the other inputs, the tensors are read by the next
 * tg_simulate and must stay valid until it has been issued. */
#define TG_ENV_SPACE 0
#define TG_LOCAL_SPACE 1
int tg_apply_rigid_body_force_tensors(tg_sim *sim, const float *forces, const float *torques, int32_t space);
/* Terrain ground (gym.add_triangle_mesh of the heightfield trimesh,
 * tasks/gogoro_new.py:164-181 with terrain_utils.convert_heightfield_to_trimesh):
 * heights [rows, cols] row-major on the HOST, vertex (i, j) at
 * (origin_x + i*horizontal_scale, origin_y + j*horizontal_scale,
 * heights[i][j]*vertical_scale), each cell split into the triangles
 * (i,j)-(i+1,j+1)-(i,j+1) and (i,j)-(i+1,j)-(i+1,j+1); friction = the mesh's
 * static/dynamic friction (combined with the shape's by averaging, like the
 * plane's).  The z = 0 plane stays (gogoro_new.py:157-159 adds both): the
 * ground is whichever surface is higher, and the plane outside the grid.
 * rows = 0 removes the terrain. */
int tg_set_heightfield(tg_sim *sim, const float *heights, int32_t rows, int32_t cols, float horizontal_scale,
                       float vertical_scale, float origin_x, float origin_y, float friction);
int tg_simulate(tg_sim *sim);
/* gym.get_sim_params / gym.set_sim_params (vec_task.py:243,650-660; the
 * reference reads the params back, edits them and writes them again for its
 * gravity randomisation).  set takes effect at the next tg_simulate; the env
 * grid (env_spacing, envs_per_row) and the asset option fix_base are fixed at
 * creation and ignored here.  solver_type must be 0 (PGS) or 1 (TGS), here
 * and in tg_sim_create (TG_ERR_ARG otherwise).
 * substeps may be 0 in set: simulate then integrates nothing and a step
 * passes the state through unchanged -- the parity tests use it to replay
 * the reference's recorded post-simulate states through the fused step. */
int tg_get_sim_params(tg_sim *sim, tg_sim_params *out);
int tg_set_sim_params(tg_sim *sim, const tg_sim_params *params);
/* refresh_rigid_body_state_tensor on the tensor from acquire_rigid_body_state_tensor
 * (IsaacGym tensor API; SURVEY §8b lists it on the boundary, the reference
 * tasks do not read it): out [N, L, 13] device, caller-owned, links in model
 * order (model.links): world origin position (3), orientation quat xyzw (4),
 * linear velocity of the link's centre of mass (3, the root-state convention),
 * angular velocity (3); from the current root and dof state, stream-ordered. */
int tg_rigid_body_states(tg_sim *sim, float *out);
/* acquire_net_contact_force_tensor: out [N, L, 3] device, caller-owned, kept alive by the caller;
 * NULL turns it off again.  Written in full by every later tg_simulate: entry
 * (e, l) is the ground's force on link l of env e (links in model order, as
 * tg_rigid_body_states), world frame, newtons, averaged over that call's
 * substeps -- 1 / (substeps h) times the sum, over the substeps and over the
 * normal and patch-friction rows of the link's shapes, of the row's
 * stored-velocity multiplier times its direction.  Links without a collision
 * shape read 0 (the call zero-fills out, stream-ordered); a simulate with 0
 * substeps writes zeros.  As in IsaacGym the tensor holds the last simulate's
 * forces until the next one; a reset does not clear it, and
 * refresh_net_contact_force_tensor has nothing to do.  While the tensor is
 * on, the task steps (tg_walk_step, tg_gogoro_step, tg_paper_step) run their
 * post-physics as a separate launch after the last simulate; the results are
 * those of that path.  Compiled-in models only: TG_ERR_MODEL for a model from
 * tg_model_jit. */
int tg_set_net_contact_force_tensor(tg_sim *sim, float *out);
/* acquire_dof_force_tensor: out [N, D] device, caller-owned, kept alive by the
 * caller; NULL turns it off again.  Written in full by every later
 * tg_simulate: entry (e, d) is the actuator's generalised force on DOF d of
 * env e (N m for a revolute joint, N for a prismatic one), the mean over that
 * call's substeps of the substep value tau.  With qd0 the DOF velocity at the
 * substep's start, qd1 the STORED velocity at its end (the bias-free one when
 * velocity iterations or TGS run, after the velocity limit -- the convention
 * of the contact tensor's multipliers) and h the substep:
 *   - POS or VEL drive, implicit in the substep's final solve:
 *       tau = te - K (qd1 - qd0) / h,
 *       te = kp (q* - q0 - h qd0) + kd (qd* - qd0),  K = h kd + h^2 kp,
 *     the implicit PD law at the end-of-substep velocity, so it includes the
 *     drive's reaction to the contact impulses;
 *   - POS or VEL drive that the effort clamp made explicit (by the Woodbury
 *     update or by the rerun): exactly +effort or -effort, the value the solve
 *     used;
 *   - EFFORT mode: clamp(actuation, +-effort) when an actuation tensor is
 *     set, else 0;
 *   - NONE mode and locked DOFs: 0.
 * The joint-limit spring and damper are NOT part of tau: it is the actuator's
 * force, which is what a torque penalty or a power estimate wants.  A
 * simulate with 0 substeps writes zeros.  As in IsaacGym the tensor holds the
 * last simulate's values until the next one; a reset does not clear it, and
 * refresh_dof_force_tensor has nothing to do.  It works together with the net
 * contact force tensor.  While the tensor is on, the task steps (tg_walk_step,
 * tg_gogoro_step, tg_paper_step) run their post-physics as a separate launch
 * after the last simulate; the results are those of that path.  Compiled-in
 * models only: TG_ERR_MODEL for a model from tg_model_jit. */
int tg_set_dof_force_tensor(tg_sim *sim, float *out);
/* refresh_jacobian_tensors on the tensor from acquire_jacobian_tensor
 * (tasks/gogoro/gogoro.py:108-114 "num_envs, num_links, 6, num_dofs + 6"):
 * out [N, L, 6, 6+D] device, caller-owned, computed on demand from the current
 * root and dof state, stream-ordered; every element is written, zeros
 * included.  The generalised velocity is
 *   u = (root linear velocity, root angular velocity, qd[0..D-1]),
 * u(0:6) exactly root_state[7:13]: the world-frame velocity of the root
 * link's centre of mass, then the world-frame angular velocity.  Columns 0..5
 * are the base, column 6+d is DOF d.  J[e, l] (6 x (6+D)) maps u to the rows
 * tg_rigid_body_states reports for link l -- the linear velocity of the
 * link's centre of mass (rows 0..2) and the angular velocity (rows 3..5),
 * world frame: J[e, l] u == rigid_body_state[e, l, 7:13].  Links in model
 * order, link 0 is the root.  With c_l the link's centre of mass, a_j the
 * world axis and p_j the anchor of DOF j's joint: a revolute column is
 * (a_j x (c_l - p_j), a_j), a prismatic one (a_j, 0); the base columns are the
 * identity and, for the angular ones, (e_k x (c_l - c_root), e_k).  A column
 * of a joint that is not on the path from the root to link l is exactly 0.0,
 * and the linear rows of the three base linear columns are exactly the
 * identity.  A locked DOF's column is its geometric column at the DOF's
 * current dof_state position, as tg_rigid_body_states takes it.  All lever
 * arms are formed relative to the root link's origin, so the result does not
 * depend on where the env sits on the grid.  With fix_base the call still
 * writes the full layout; IsaacGym's fixed-base tensor is the view
 * J[:, 1:, :, 6:]. */
int tg_jacobians(tg_sim *sim, float *out);
/* refresh_mass_matrix_tensors on the tensor from acquire_mass_matrix_tensor
 * (tasks/franka_cube_stack.py:393,441): out [N, 6+D, 6+D] device,
 * caller-owned, on demand from the current root and dof state,
 * stream-ordered; every element is written, zeros included.  In the
 * generalised velocity u of tg_jacobians, with Jv_l / Jw_l the linear and
 * angular rows of J[e, l]:
 *   H = sum_l s_l (m_l Jv_l^T Jv_l + Jw_l^T R_l I_l R_l^T Jw_l)
 *       + diag(0_6, armature),
 * s_l the env's body mass scale (tg_set_body_mass_scale_indexed: it scales
 * mass and inertia together, as the step's composites do), I_l the link
 * inertia about its centre of mass, armature the env's TG_PROP_ARMATURE row.
 * H[0:6, 0:6] is the whole body's inertia at the root link's centre of mass.
 * Locked DOFs are ordinary rows and columns, at their dof_state position; the
 * step's dynamics are those of H with the locked rows and columns removed
 * (the locked DOFs at the centre of their windows).  H is symmetric bit for
 * bit.  With fix_base IsaacGym's tensor is the view H[:, 6:, 6:]. */
int tg_mass_matrices(tg_sim *sim, float *out);
/* Damped-least-squares end-effector IK, the hand IK of
 * tasks/gogoro/gogoro.py:381-427 in one kernel: for K chains per env, the pose
 * error of a point on a link to a goal, the step
 *   u = J^T (J J^T + lambda^2 I)^-1 dpose
 * on the chain's own Jacobian columns, and optionally the position targets
 * q + u.  On demand, stream-ordered, computed from the current root and dof
 * state; nothing else of the sim is read and nothing of it is written.  The
 * chains array is HOST memory, read during the call and not retained.
 *
 * Controlled point and rows, chain k of env e, l = chains[k].link: the
 * controlled point is x = o_l + R_l offset, o_l the link ORIGIN -- the
 * position tg_rigid_body_states reports in [0:3] -- and R_l the link's
 * rotation; not the centre of mass the linear rows of tg_jacobians use.  Jv is
 * the Jacobian of x: a revolute column is a_j x (x - p_j), a prismatic one a_j
 * (a_j the world axis, p_j the anchor of the DOF's joint); Jw is the angular
 * Jacobian, a_j for a revolute column and 0 for a prismatic one.  Only the
 * chain's DOF columns enter, the base is held fixed.  A chain DOF whose joint
 * is not on the path from the root to the link has an exactly-0 column, so its
 * dq is exactly 0.0 (the off-path rule of tg_jacobians).  A locked DOF is an
 * ordinary column at its dof_state position.
 *
 * Pose error (orientation_error, gogoro.py:605-608):
 *   err[0:3] = (goal_pos - root_pos) - (x - root_pos),
 * both differences formed relative to the root link's origin before they are
 * subtracted, so the error does not depend on where the env sits on the grid;
 *   err[3:6] = vec(q_goal (x) conj(q_l)) s, s = +1 if the product's w >= 0 and
 * -1 otherwise, quaternions xyzw, q_goal normalised by the kernel.  With
 * goal_quat NULL the system has the 3 position rows only and err[3:6] is
 * written as 0.
 *
 * Solve: y = (J J^T + lambda^2 I)^-1 err by Cholesky (6 x 6, or 3 x 3 without
 * goal_quat; SPD since lambda > 0), dq[e, k, c] = (J^T y)_c for c < num_dofs
 * and exactly 0.0 for the padding c >= num_dofs: every element of dq and err
 * is written.
 *
 * Position targets: with pos_targets, for every DOF d that appears in at least
 * one chain, pos_targets[e, d] = q[e, d] + sum of dq[e, k, c] over all (k, c)
 * with dofs[c] == d, in ascending (k, c) order, no atomics; chains may share a
 * DOF.  No other element of pos_targets is touched, and the targets are not
 * clamped to the joint limits.
 *
 * TG_ERR_ARG (message "tg_ik_dls: ...") for null chains or goal_pos,
 * num_chains outside 1..TG_IK_MAX_CHAINS, a link outside [0, L), num_dofs
 * outside 1..TG_IK_MAX_DOFS, a DOF outside [0, D), a DOF twice in one chain,
 * damping not > 0 or not finite, or dq, err and pos_targets all NULL.  Every
 * model, run-time (tg_model_jit) ones included. */
#define TG_IK_MAX_CHAINS 8
#define TG_IK_MAX_DOFS   8
typedef struct tg_ik_chain {
    int32_t link;                   /* end-effector link, model order (tg_rigid_body_states) */
    int32_t num_dofs;               /* 1..TG_IK_MAX_DOFS */
    int32_t dofs[TG_IK_MAX_DOFS];   /* DOF indices the solve may move; entries >= num_dofs ignored */
    float   offset[3];              /* controlled point in the link frame (0 = the link origin) */
} tg_ik_chain;                      /* 52 bytes */
int tg_ik_dls(tg_sim *sim, const tg_ik_chain *chains /* HOST */, int32_t num_chains,
              const float *goal_pos,   /* [N, K, 3] device, world frame as tg_rigid_body_states */
              const float *goal_quat,  /* [N, K, 4] xyzw device, or NULL: position only (3 rows) */
              float damping,           /* lambda > 0 */
              float *dq,               /* [N, K, TG_IK_MAX_DOFS] device or NULL */
              float *err,              /* [N, K, 6] device or NULL */
              float *pos_targets);     /* [N, D] device or NULL */
/* Operational-space control, _compute_osc_torques of
 * tasks/franka_cube_stack.py:602-628 in one kernel: for K chains per env, the
 * joint torques
 *   tau = J^T Lambda (kp err - kd v) + (H_c a - J^T Lambda (J a)),
 *   Lambda = (J H_c^-1 J^T + lambda^2 I)^-1,
 * on the chain's own Jacobian columns and the chain's own block of the mass
 * matrix, and optionally their clamped sum into an actuation tensor.  On
 * demand, stream-ordered, computed from the current root and dof state, the
 * env's body mass scales and its TG_PROP_ARMATURE and TG_PROP_EFFORT rows;
 * nothing of the sim is written.  The chains array and the gains are HOST
 * memory, read during the call and not retained.  The chains are tg_ik_dls's
 * tg_ik_chain records.  Chain k of env e has nd = num_dofs columns and R = 6
 * rows, or R = 3 (the position rows) with goal_quat NULL.
 *
 * J (R x nd), the controlled point x and err are exactly tg_ik_dls's: the
 * point is x = o_l + R_l offset on the link ORIGIN, the base is held fixed, a
 * chain DOF whose joint is off the link's path has an exactly-0 column, a
 * locked DOF is an ordinary column at its dof_state position, q_goal is
 * normalised by the kernel, and err[3:6] is written as 0 without goal_quat.
 *
 * H_c (nd x nd) = H[6 + dofs[i], 6 + dofs[j]] with H as tg_mass_matrices
 * defines it: the env's body mass scale and its TG_PROP_ARMATURE row included,
 * locked DOFs ordinary rows.  It is the reference's mm[:, :7, :7], the inertia
 * seen with the base and every non-chain joint held.
 *
 * v = J qd_c, qd_c the chain DOFs' dof_state velocities: the velocity of the
 * controlled point with the base held, whatever the root's own velocity is.
 * With a fixed base it equals the reference's eef_vel.
 *
 * Lambda = (J H_c^-1 J^T + lambda^2 I)^-1, lambda = gains.damping > 0, both
 * inverses by Cholesky (H_c is SPD, and so is the R x R matrix since lambda >
 * 0); the reference is lambda = 0.
 *
 * Null space, with q_rest only: a = kp_null w(q_rest - q) - kd_null qd over
 * the chain's DOFs, w(x) = x - 2 pi floor((x + pi) / (2 pi)) for a revolute
 * DOF (the reference's % (2 pi) wrap) and w(x) = x for a prismatic one;
 * tau += H_c a - J^T Lambda (J a).  This is the reference's
 * (I - J^T Jbar) H a with Jbar = Lambda J H_c^-1, identical for any lambda.
 * kp_null and kd_null are ignored without q_rest.
 *
 * tau[e, k, c] is the torque of chain k's column c and exactly 0.0 for the
 * padding c >= num_dofs: every element of tau and err is written.  Without
 * q_rest an off-path column's tau is exactly 0.0.  tau is not clamped.
 *
 * efforts: for every DOF d that appears in at least one chain, efforts[e, d] =
 * clamp(sum of tau[e, k, c] over all (k, c) with dofs[c] == d, in ascending
 * (k, c) order, no atomics; -TG_PROP_EFFORT[e, d], +TG_PROP_EFFORT[e, d]), the
 * reference's tensor_clamp to the effort limits; chains may share a DOF.  No
 * other element of efforts is touched.  Passing the sim's live dof_actuation
 * tensor (tg_state_view) is the intended use: the next tg_simulate applies it
 * to the chain DOFs that are in EFFORT mode.
 *
 * TG_ERR_ARG (message "tg_osc: ...") for every chain error tg_ik_dls reports
 * (null chains or goal_pos, num_chains outside 1..TG_IK_MAX_CHAINS, a link
 * outside [0, L), num_dofs outside 1..TG_IK_MAX_DOFS, a DOF outside [0, D), a
 * DOF twice in one chain), null gains, damping not > 0 or not finite, kp, kd,
 * kp_null or kd_null negative or not finite, or tau, err and efforts all NULL.
 * Every model, run-time (tg_model_jit) ones included. */
typedef struct tg_osc_gains {      /* HOST, read during the call, one set for all chains */
    float kp, kd;                  /* task space (reference: 150, 2 sqrt(kp)) */
    float kp_null, kd_null;        /* null space (reference: 10, 2 sqrt(kp_null)); ignored without q_rest */
    float damping;                 /* lambda > 0, regularises the task-space inertia */
} tg_osc_gains;                    /* 20 bytes */
int tg_osc(tg_sim *sim, const tg_ik_chain *chains /* HOST */, int32_t num_chains,
           const float *goal_pos,   /* [N, K, 3] device, world */
           const float *goal_quat,  /* [N, K, 4] xyzw device or NULL: 3 position rows only */
           const float *q_rest,     /* [N, D] device or NULL: no null-space term */
           const tg_osc_gains *gains,
           float *tau,              /* [N, K, TG_IK_MAX_DOFS] device or NULL */
           float *err,              /* [N, K, 6] device or NULL */
           float *efforts);         /* [N, D] device or NULL */
/* Inverse dynamics by one recursive Newton-Euler pass in one kernel: the
 * generalised force tau = H a + h(q, u) of the equation of motion H u' + h =
 * tau, in exactly the coordinates of tg_jacobians and tg_mass_matrices, and
 * optionally its DOF entries clamped into an actuation tensor: gravity and
 * Coriolis compensation for effort-mode drives (tg_osc has none), computed-
 * torque control, feed-forward for the PD drives.  On demand, stream-ordered,
 * computed from the current root and dof state, the sim's current gravity
 * (tg_set_gravity included), the env's body mass scales and its
 * TG_PROP_ARMATURE and TG_PROP_EFFORT rows; nothing of the sim is written.
 * dofs is HOST memory, read during the call and not retained (it travels to
 * the kernel as a bitmask in its arguments).
 *
 * Let u, J[e, l] (Jv, Jw), s_l, m_l, I_l, R_l and H be exactly those of
 * tg_jacobians and tg_mass_matrices -- in particular u(0:6) = root_state[7:13],
 * the base linear velocity being that of the root link's centre of mass -- and
 * g the gravity vector.  Then
 *   tau = H a + sum_l s_l [ Jv_l^T m_l (ab_l - [GRAVITY] g)
 *                           + Jw_l^T (R_l I_l R_l^T alb_l + w_l x (R_l I_l R_l^T w_l)) ]
 * where ab_l and alb_l are the velocity-product accelerations of link l: the
 * time derivatives of Jv_l u and Jw_l u with u' held at 0, and w_l = Jw_l u.
 * Without TG_ID_VELOCITY u is taken as 0, so ab, alb and w all vanish.  a is
 * accel, 0 when accel is NULL; H a includes the armature on the diagonal.
 *
 * So tau[0:3] is the net force, tau[3:6] the net moment about the root link's
 * centre of mass, tau[6 + d] DOF d's generalised force.  Locked DOFs are
 * ordinary entries at their dof_state position and velocity, as in H.  All
 * lever arms are formed relative to the root link's origin: the result does
 * not depend on where the env sits on the grid.  Every element of tau is
 * written.  With fix_base the call still writes the full layout: tau[:, 6:]
 * with u(0:6) = 0 is the fixed-base result, rows 0..5 are then the reaction at
 * the base.
 *
 * efforts: for every selected DOF d (dofs[0..num_dofs); every DOF with dofs
 * NULL and num_dofs 0), with t = tau[6 + d]:
 *   accumulate == 0:  efforts[e, d] = clamp(t, -TG_PROP_EFFORT[e, d], +TG_PROP_EFFORT[e, d])
 *   accumulate != 0:  efforts[e, d] = clamp(efforts[e, d] + t, -TG_PROP_EFFORT[e, d], +TG_PROP_EFFORT[e, d])
 * No other element of efforts is touched.  The intended use is tg_osc with
 * efforts = the sim's live dof_actuation tensor, then this call with the same
 * tensor, the chains' DOFs and accumulate = 1 on the same stream; note that
 * this clamps twice: tg_osc clamps its own sum, and this call clamps that
 * clamped value plus t.
 *
 * TG_ERR_ARG (message "tg_inverse_dynamics: ...") for a null sim, terms
 * outside 0..3, terms == 0 with accel NULL, tau and efforts both NULL,
 * num_dofs outside 0..D, dofs NULL with num_dofs > 0, a DOF outside [0, D), a
 * DOF listed twice (and efforts on a model of more than 256 DOFs).  Every
 * model, run-time (tg_model_jit) ones included. */
#define TG_ID_GRAVITY  1   /* the -g term */
#define TG_ID_VELOCITY 2   /* Coriolis / centrifugal terms */
int tg_inverse_dynamics(tg_sim *sim, int32_t terms,   /* TG_ID_* mask, may be 0 only with accel */
                        const float *accel,           /* [N, 6+D] device or NULL (= 0) */
                        float *tau,                   /* [N, 6+D] device or NULL */
                        float *efforts,               /* [N, D] device or NULL */
                        const int32_t *dofs /* HOST */, int32_t num_dofs, /* NULL, 0: every DOF */
                        int32_t accumulate);          /* 0: efforts = clamp(t); 1: efforts = clamp(efforts + t) */
/* Centroidal quantities of the floating-base robot in one kernel: the whole-
 * body centre of mass (CoM) and its velocity, the angular momentum about the
 * CoM, the total mass and the centroidal inertia (state), the centroidal
 * momentum matrix A with h_G = A u (matrix) and the momentum-rate bias A' u
 * (bias): what CoM height and velocity rewards, angular-momentum
 * regularisation, capture-point termination, CoM-Jacobian balance IK and
 * momentum-based whole-body control are built from.  On demand, stream-ordered,
 * computed from the current root and dof state and the env's body mass scales
 * (tg_set_body_mass_scale_indexed); nothing of the sim is written and nothing
 * is kept on the host between calls.  Each output is optional: a NULL output
 * is not touched and its part of the work is skipped; every element of every
 * non-NULL output is written.
 *
 * Let u, J[e, l] = (Jv_l; Jw_l), c_l, R_l, I_l and s_l be exactly those of
 * tg_jacobians and tg_mass_matrices, m'_l = s_l m_l and I'_l = s_l R_l I_l
 * R_l^T.  Then
 *   M = sum_l m'_l,   c = sum_l m'_l c_l / M,
 *   A = sum_l [ m'_l Jv_l ; I'_l Jw_l + (c_l - c) x m'_l Jv_l ]     (6 x (6 + D))
 * rows 0..2 of A give the linear momentum, rows 3..5 the angular momentum
 * about c, world axes; A[0:3] / M is the CoM Jacobian.
 *
 * state[e], TG_CENTROIDAL_STATE = 16 floats:
 *   [0:3]   c, in the world frame of tg_rigid_body_states
 *   [3:6]   c', the CoM velocity; the linear momentum is M c'
 *   [6:9]   k, the angular momentum about c
 *   [9]     M
 *   [10:16] I_G = sum_l (I'_l + m'_l (|d|^2 1 - d d^T)), d = c_l - c, in the
 *           order xx yy zz xy xz yz of link_inertia
 * so that A u = (M c', k) by definition.
 *
 * matrix[e] = A, row-major, in the column layout of tg_jacobians: base columns
 * 0..5, DOF d at column 6 + d.  Armature does not enter.  A locked DOF is an
 * ordinary column at its dof_state position, and its dof_state velocity enters
 * the state (the rule of tg_jacobians).  A[0:3, 0:3] = M 1 with exact 0.0 off
 * the diagonal and A[3:6, 0:3] = 0.0 (it vanishes identically, c being the
 * CoM) are written exactly; mathematically A[3:6, 3:6] = I_G and A[0:3, 3:6] =
 * -M [c - c_root]x, c_root the root link's centre of mass.  With fix_base the
 * call still writes the full layout: matrix[:, :, 6:] is the fixed-base view.
 *
 * bias[e] = A' u, the momentum rate at u' = 0 without gravity, so that h_G' =
 * A u' + bias: the net force and moment of the links' velocity-product
 * inertial forces, the moment taken about c.  It equals the base rows of
 * tg_inverse_dynamics(TG_ID_VELOCITY) with the moment moved from the root
 * link's centre of mass to c.
 *
 * All lever arms are formed relative to the root link's origin; c is that
 * relative CoM plus the root position, added last: every output other than
 * state[0:3] is bit-identical wherever the env sits on the grid.  The outputs
 * a call shares with a call that asks for fewer or more of them are
 * bit-identical too.
 *
 * TG_ERR_ARG (message "tg_centroidal: ...") for a null sim or state, matrix
 * and bias all NULL.  Every model, run-time (tg_model_jit) ones included. */
#define TG_CENTROIDAL_STATE 16
int tg_centroidal(tg_sim *sim,
                  float *state,    /* [N, TG_CENTROIDAL_STATE] device or NULL */
                  float *matrix,   /* [N, 6, 6+D] device or NULL */
                  float *bias);    /* [N, 6] device or NULL */
/* Contact-consistent inverse dynamics in one kernel: the joint torques of a
 * floating-base robot that stands on some of its links -- gravity compensation
 * for a standing or walking humanoid, the feed-forward of a whole-body
 * controller -- and the contact wrenches that go with them, from which the
 * caller reads each foot's vertical load, centre of pressure and friction use.
 * On demand, stream-ordered, computed from the current root and dof state, the
 * sim's current gravity, the env's body mass scales and its TG_PROP_ARMATURE
 * and TG_PROP_EFFORT rows; nothing of the sim is written.  contacts and dofs
 * are HOST memory, read during the call and not retained (they travel to the
 * kernel by value in its arguments).
 *
 * Let b = H a + h be exactly the tau of tg_inverse_dynamics for the same terms
 * and accel: the same coordinates, gravity, mass scales and armature.  Contact
 * k of K is a point fixed on link l_k:
 *   p_k = o_l + R_l offset_k, offset_k in the link frame (the convention of
 *         tg_ik_chain.offset), o_l the link's origin;
 *   r_k = p_k - c_root, c_root the root link's centre of mass;
 *   Jp_k, the 6 x (6 + D) Jacobian of the point: the linear velocity of p_k
 *         and the angular velocity of the link, Jv_l - [p_k - c_l]x Jw_l
 *         stacked on Jw_l from the rows of tg_jacobians (c_l the link's com);
 *   G_k = Jp_k[:, 0:6]^T = [[1, 0], [[r_k]x, 1]].
 * Each contact carries a wrench lambda_k = (f_k, n_k): the force and moment
 * the environment exerts on the robot, world axes, the moment about p_k.  The
 * call chooses the wrenches that balance the base rows at least weighted cost:
 *   minimise  sum_k (|f_k|^2 + |n_k|^2 / l^2) / s_k   subject to   sum_k G_k lambda_k = b[0:6]
 * s_k >= 0 is the per-env load share of contact k (share [N, K]; NULL: all
 * ones; negative values are taken as 0) and l = moment_arm > 0, in metres: a
 * moment n costs as much as a force n / l.  In closed form, with
 * Dm = diag(1, 1, 1, l^2, l^2, l^2):
 *   A = sum_k s_k G_k Dm G_k^T     (6 x 6; SPD whenever some s_k > 0, G_k being invertible)
 *   y = A^-1 b[0:6]
 *   f_k = s_k (y_f + y_n x r_k)
 *   n_k = s_k l^2 y_n
 *   tau[6 + d] = b[6 + d] - sum_k Jp_k[:, 6 + d]^T lambda_k   (the armature is already in b)
 *   tau[0:6]   = b[0:6] - sum_k G_k lambda_k
 * tau[0:6] is the part of the base wrench that the contacts do not carry: 0 up
 * to rounding for an env with some s_k > 0.  (The minimiser does not depend on
 * the point the moments are taken about; the kernel takes them about the
 * share-weighted mean of the contact points, where A is block diagonal.)
 *
 * A contact with s_k = 0 gets a wrench of exactly 0.0, and such an env's other
 * outputs equal those of a call without that contact: a swing foot.  An env
 * with every s_k = 0 is airborne: no solve is made, every lambda_k is 0.0 and
 * tau equals b, the plain inverse dynamics.
 *
 * The distribution is a least-squares one.  It knows nothing of unilateral
 * contact, friction cones or the foot's outline.  The caller judges
 * feasibility from the returned wrenches (f_z > 0, |f_xy| <= mu f_z, the centre
 * of pressure (-n_y / f_z, n_x / f_z) inside the sole) and steers it with
 * share.
 *
 * wrench[e, k] = (f_k, n_k).  terms, accel, efforts, dofs, num_dofs and
 * accumulate mean exactly what they mean in tg_inverse_dynamics, with t =
 * tau[6 + d] of this call: the clamp to TG_PROP_EFFORT, the limit of 256 DOFs
 * for efforts, and no other element of efforts is touched.  Every element of
 * every non-NULL output is written; with fix_base the full layout is written
 * too.  All lever arms are formed relative to the root link's origin: the
 * result is bit-identical wherever the env sits on the grid.
 *
 * TG_ERR_ARG (message "tg_contact_inverse_dynamics: ...") for a null sim, null
 * contacts, num_contacts outside 1..TG_CID_MAX_CONTACTS, a link outside [0, L),
 * a link listed twice, moment_arm not finite or <= 0, tau, wrench and efforts
 * all NULL, and every argument error of tg_inverse_dynamics on the arguments
 * the two share (terms outside 0..3, terms == 0 with accel NULL, num_dofs
 * outside 0..D, dofs NULL with num_dofs > 0, a DOF outside [0, D), a DOF
 * listed twice, efforts on a model of more than 256 DOFs).  A rejected call
 * launches nothing.  Every model, run-time (tg_model_jit) ones included. */
#define TG_CID_MAX_CONTACTS 4          /* both feet and both hands */
typedef struct tg_contact_frame {      /* HOST, read during the call */
    int32_t link;
    float offset[3];                   /* the contact point in the link frame */
} tg_contact_frame;                    /* 16 bytes */
int tg_contact_inverse_dynamics(tg_sim *sim, const tg_contact_frame *contacts /* HOST */, int32_t num_contacts,
                                const float *share,   /* [N, K] device or NULL (= 1) */
                                float moment_arm, int32_t terms, const float *accel /* [N, 6+D] or NULL */,
                                float *tau,           /* [N, 6+D] device or NULL */
                                float *wrench,        /* [N, K, 6] device or NULL */
                                float *efforts,       /* [N, D] device or NULL */
                                const int32_t *dofs /* HOST */, int32_t num_dofs, int32_t accumulate);
/* acquire_force_sensor_tensor (with create_asset_force_sensor implied): the
 * measured counterpart of the wrenches tg_contact_inverse_dynamics predicts.
 * Up to TG_FS_MAX_SENSORS sensors per env; sensor k is the point
 *   p_k = o_l + R_l offset_k
 * on link l_k, the convention of tg_contact_frame and tg_ik_chain.offset, and
 * the same link may carry several sensors at different offsets.  The sensor
 * array is read during the call and copied.  out [N, S, 6] device,
 * caller-owned, kept alive by the caller: out[e, k] = (f, n), newtons and
 * newton metres, the GROUND REACTION on the sensor's link -- the force the
 * ground exerts on the link's collision shapes and its moment about p_k.  It
 * is not IsaacGym's joint-transmitted constraint force: there is no gravity
 * or inertial part in it and nothing from the links further down the chain.
 *
 * Written in full by every later tg_simulate and averaged over that call's
 * substeps.  Per substep of length h, over the rows j of the shapes on link
 * l_k -- the normal rows, the two patch-friction rows and the torsion row --
 * with lambda_j the row's stored-velocity multiplier, d_j its direction, x_j
 * its point of application (the support point of a normal row, the patch's
 * friction anchor of a friction row; the torsion row has d_j = 0) and t_j the
 * torsion row's pure moment (the patch normal; 0 for every other row):
 *   f = (1 / h) sum_j lambda_j d_j
 *   n = (1 / h) sum_j lambda_j ((x_j - p_k) x d_j + t_j)
 * p_k is posed from the state the substep starts from, as the rows are.  f is
 * the very sum the net contact force tensor holds for the link (bit for bit
 * in TG_ENV_SPACE); the moment is new, and the torsion row, which carries no
 * force, enters it.
 *
 * space: TG_ENV_SPACE gives world axes, the convention of the wrench output of
 * tg_contact_inverse_dynamics; TG_LOCAL_SPACE the link's own axes, rotated per
 * substep with the R_l the substep starts from -- how IsaacGym's sensors read,
 * and the centre of pressure (-n_y / f_z, n_x / f_z) of a sole whose normal is
 * the link's z then comes out in sole coordinates whatever the yaw.
 *
 * A sensor on a link without collision shapes reads zeros, and so does every
 * sensor after a simulate with 0 substeps.  The call zero-fills out,
 * stream-ordered; the tensor then holds the last simulate's values until the
 * next one, a reset does not clear it, and refresh_force_sensor_tensor has
 * nothing to do.  out == NULL or num_sensors == 0 turns it off.  It works
 * together with the net contact force and DOF force tensors (one launch for
 * any combination).  While it is on, the task steps (tg_walk_step,
 * tg_gogoro_step, tg_paper_step) run their post-physics as a separate launch
 * after the last simulate; the states never depend on it.
 *
 * TG_ERR_ARG (message "tg_set_force_sensor_tensor: ...") for a null sim,
 * num_sensors outside 0..TG_FS_MAX_SENSORS, null sensors with num_sensors > 0,
 * a link outside [0, L), a non-finite offset, space outside {0, 1} and a
 * non-null out with num_sensors == 0; TG_ERR_MODEL for a model from
 * tg_model_jit.  A rejected call changes nothing. */
#define TG_FS_MAX_SENSORS 8
int tg_set_force_sensor_tensor(tg_sim *sim, const tg_contact_frame *sensors /* HOST */, int32_t num_sensors,
                               int32_t space /* TG_ENV_SPACE | TG_LOCAL_SPACE */, float *out /* [N, S, 6] device */);
/* The ground under the robot in one kernel: terrain heights, and optionally
 * the surface normals, at a pattern of points about up to TG_SCAN_MAX_FRAMES
 * link frames -- the height scan around the base that terrain locomotion
 * observes (measured_heights: get_heights with init_height_points,
 * tasks/anymal_terrain.py:501-536, entering the observation at :301-302), and,
 * with the feet as frames, the swing-foot clearance and the slope under a
 * sole.  On demand, stream-ordered, from the current root and dof state and
 * the heightfield the sim holds at the time of the call (tg_set_heightfield; a
 * later change, removal with rows = 0 included, is seen by the next call);
 * nothing of the sim is written and nothing is kept on the host between calls.
 * A NULL output is not touched; every element of every non-NULL output is
 * written.
 *
 * Frame f is the point
 *   p_f = o_l + R_l offset_f
 * on link l_f, the convention of tg_contact_frame, tg_set_force_sensor_tensor
 * and tg_ik_chain.offset, o_l and R_l those of tg_rigid_body_states (world
 * coordinates, the ones the contacts' ground takes); a link may appear in
 * several frames.  points [P, 2] is one pattern for every env and frame.  The
 * sample of pattern point (a, b) = points[k] is at the world position
 *   (x, y) = (p_f.x, p_f.y) + d.xy
 *   TG_SCAN_WORLD   d = (a, b, 0)
 *   TG_SCAN_LINK    d = R_l (a, b, 0): laid out in the link's own axes, then
 *                   dropped vertically
 *   TG_SCAN_YAW     d = Rz(psi) (a, b, 0), Rz(psi) the reference's
 *                   quat_apply_yaw: the link's quaternion with x and y zeroed,
 *                   normalised.  (cos psi, sin psi) is (R00 + R11, R10 - R01)
 *                   normalised; the identity when both are 0
 * and h, n there are
 *   TG_SCAN_SURFACE the surface the contacts feel, by the very function the
 *                   step kernel's contact rows call (ground_at): the triangle
 *                   rule of tg_set_heightfield or the z = 0 plane, whichever is
 *                   higher, the plane outside the grid, n the unit normal of
 *                   the triangle (e_z on the plane).  Without a heightfield
 *                   h = 0 and n = e_z
 *   TG_SCAN_CELL    the reference's rule (anymal_terrain.py:524-536):
 *                   u = (x - ox) / hs, i = clamp(trunc(u), 0, rows - 2), j
 *                   likewise from y, h = vs min(hf[i][j], hf[i+1][j+1]).  No
 *                   plane; a point off the grid reads the border cell.
 *                   Without a heightfield h = 0.  There is no normal: normals
 *                   must be NULL
 *
 * heights[e, f, k] = h with params.relative == 0; otherwise
 *   heights[e, f, k] = clamp(p_f.z - bias - h, lo, hi) * scale
 * which is line 302 of the reference in the same launch (bias 0.5, clip +-1,
 * height_meas_scale) and, at a foot, its clearance.  normals[e, f, k] = n.
 * bias, lo, hi and scale are not read with relative == 0.
 *
 * The link poses are formed relative to the root link's origin and the root
 * position is added last, as in tg_centroidal; p_f agrees with
 * tg_rigid_body_states to rounding.  Envs do not interact: an env's results
 * do not depend on the other envs' states.
 *
 * TG_ERR_ARG (message "tg_height_scan: ...") for a null sim, frames, points or
 * params, num_frames outside 1..TG_SCAN_MAX_FRAMES, num_points outside
 * 1..TG_SCAN_MAX_POINTS, a link outside [0, L), a non-finite offset, surface
 * outside {0, 1}, align outside {0, 1, 2}, relative != 0 with a non-finite
 * bias or scale or without lo <= hi, normals together with TG_SCAN_CELL, and
 * heights and normals both NULL.  A rejected call launches nothing.  Every
 * model, run-time (tg_model_jit) ones included. */
#define TG_SCAN_MAX_FRAMES 8
#define TG_SCAN_MAX_POINTS 1024
#define TG_SCAN_SURFACE 0   /* the trimesh surface the contacts feel (ground_at) */
#define TG_SCAN_CELL    1   /* the reference's rule, anymal_terrain.py:524-536   */
#define TG_SCAN_YAW   0     /* pattern turned by the frame link's heading        */
#define TG_SCAN_WORLD 1     /* pattern in world axes                             */
#define TG_SCAN_LINK  2     /* pattern in the link's own axes, then dropped vertically */
typedef struct tg_scan_params {   /* HOST, read during the call */
    int32_t surface, align, relative;
    float bias, lo, hi, scale;    /* used when relative != 0 */
} tg_scan_params;                 /* 28 bytes */
int tg_height_scan(tg_sim *sim, const tg_contact_frame *frames /* HOST */, int32_t num_frames,
                   const float *points /* [P, 2] device */, int32_t num_points,
                   const tg_scan_params *params /* HOST */,
                   float *heights /* [N, F, P] device or NULL */,
                   float *normals /* [N, F, P, 3] device or NULL */);
/* The inertial measurement unit in one kernel: orientation, projected gravity,
 * body-frame velocities, gyro and accelerometer readings at up to
 * TG_IMU_MAX_SENSORS link frames -- what the reference's paper task observes as
 * "imu" roll, yaw and their rates with an IMU noise and an IMU offset
 * (tasks/gogoro_realistic_turning_sim_paper.py:55-67, :525-531) and what every
 * legged sim-to-real policy starts from.  On demand, stream-ordered, from the
 * current root and dof state and the sim's gravity at the time of the call
 * (tg_set_gravity is honoured); nothing of the sim is written and the library
 * keeps nothing between calls: no host cache, no hidden step counter.  The
 * previous velocities an accelerometer needs live in the caller-owned history
 * tensor.
 *
 * Sensor s is the point
 *   p_s = o_l + R_l offset_s
 * on link l_s, the convention of tg_contact_frame, tg_set_force_sensor_tensor
 * and tg_height_scan; a link may appear in several sensors.  Its axes are the
 * link's.  From the current state
 *   R   = R_l, the link's rotation (link to world)
 *   w   = the link's world angular velocity, as tg_rigid_body_states reports it
 *   v   = the world velocity of the material point p_s: the link origin's
 *         velocity plus w x R_l offset_s.  (root_state[7:10] is the velocity
 *         of the root link's centre of mass, as in tg_rigid_body_states.)
 * and with g the sim's gravity, out[e, s, 0:TG_IMU_WIDTH] is
 *   0:4    the link's world quaternion xyzw, as tg_rigid_body_states reports it
 *   4:7    gravity_b = R^T g / |g|, zero when |g| = 0
 *   7:10   lin_vel_b = R^T v
 *   10:13  ang_vel_b = R^T w + bias[e, s, 0:3] + gyro_noise * n[0:3]
 *   13:16  lin_acc_b = R^T (a - g) + bias[e, s, 3:6] + accel_noise * n[3:6],
 *          the specific force: +|g| along world up at rest, 0 in free fall
 *   16:19  ang_acc_b = R^T alpha
 *   19     valid: 1.0 where a and alpha were differenced, else 0.0
 * a = (v - v_prev) / dt and alpha = (w - w_prev) / dt, v_prev and w_prev from
 * history [N, S, TG_IMU_HISTORY]: v world in slots 0:3, w world in slots 3:6,
 * the valid flag in slot 6, slot 7 written 0.  a = alpha = 0 and valid = 0, so
 * that the accelerometer reads -R^T g, whenever history is NULL, the history's
 * flag is not 1.0, or reset[e] != 0.  After forming the outputs the call writes
 * the current true (noise-free, bias-free) v, w and the flag 1.0 into history,
 * reset envs included; the history is read before it is written.
 *
 * dt is the sim time since the history was written; the caller states it.
 * reset is [N] int64 on the device or NULL, the dtype of VecTask.reset_buf and
 * tg_walk_buffers.reset_buf; bias is [N, S, 6] on the device or NULL.  n are
 * standard normals, drawn only when a sigma is non-zero: Philox block
 * 3 (e S + s) + j, j = 0..2, has counter (block, counter lo, counter hi, 0) and
 * key seed, and its two values gauss(x, y), gauss(z, w) are n[2j], n[2j+1] --
 * exactly the blocks and functions of tg_rng_fill kind 2 with n = 3 N S.
 *
 * The link poses are formed relative to the root link's origin; no absolute
 * position enters any output, so every output is bit-identical wherever the
 * env stands.  Envs do not interact.  Every element of out is written.
 *
 * TG_ERR_ARG (message "tg_imu: ...") and nothing launched, in this order, for
 * null sensors, params or out, num_sensors outside 1..TG_IMU_MAX_SENSORS, a
 * negative link, a non-finite offset, a non-finite or negative sigma, a history
 * given with a dt that is not finite and > 0, a null sim, a link >= L: what
 * needs no sim first, then the sim, then the links.  Every model, run-time
 * (tg_model_jit) ones included. */
#define TG_IMU_MAX_SENSORS 8
#define TG_IMU_WIDTH 20     /* floats per sensor reading   */
#define TG_IMU_HISTORY 8    /* floats per sensor's history */
typedef struct tg_imu_params {   /* HOST, read during the call */
    float dt, gyro_noise, accel_noise;
    int32_t pad;
    uint64_t seed, counter;
} tg_imu_params;                 /* 32 bytes */
int tg_imu(tg_sim *sim, const tg_contact_frame *sensors /* HOST */, int32_t num_sensors,
           const tg_imu_params *params /* HOST */, const float *bias /* [N, S, 6] device or NULL */,
           const int64_t *reset /* [N] device or NULL */, float *history /* [N, S, 8] device or NULL */,
           float *out /* [N, S, 20] device */);
/* Range sensing in one kernel: the distance along each ray of a pattern, and
 * optionally the surface normal where it lands, cast from up to
 * TG_RAY_MAX_FRAMES link frames against the ground -- a lidar ring, a
 * forward-looking depth image, anything tg_height_scan's straight-down lookup
 * cannot give.  On demand, stream-ordered, from the current root and dof state
 * and the heightfield the sim holds at the time of the call
 * (tg_set_heightfield; a later change, removal with rows = 0 included, is seen
 * by the next call); nothing of the sim is written and nothing is kept on the
 * host between calls.  A NULL output is not touched; every element of every
 * non-NULL output is written.
 *
 * Frame f is the point
 *   p_f = o_l + R_l offset_f
 * on link l_f, as in tg_height_scan (tg_contact_frame; o_l and R_l those of
 * tg_rigid_body_states); a link may appear in several frames.  rays [R, 6] is
 * one pattern for every env and frame: rays[k] = (s_k, d_k), a start offset
 * and a direction in the pattern's axes.  With the alignment matrix
 *   TG_RAY_LINK   A = R_l, the link's own axes (its full 3-D rotation)
 *   TG_RAY_YAW    A = Rz(psi), tg_height_scan's rule: (cos psi, sin psi) is
 *                 (R00 + R11, R10 - R01) normalised; the identity when both
 *                 are 0
 *   TG_RAY_WORLD  A = I
 * the world ray is
 *   x(t) = p_f + A s_k + t A d_k,   t >= 0.
 * d_k is NOT normalised by the call and t is the ray parameter: with unit
 * directions t is the range; with a pinhole pattern scaled to d.x = 1 it is
 * the depth along the optical axis.  max_range bounds t.
 *
 * The ground is the solid under the surface the contacts feel.  H(x, y) is the
 * triangle height of tg_set_heightfield -- the cell split and the fu >= fv rule
 * of ground_at -- defined on the closed grid rectangle
 * [ox, ox + (rows - 1) hs] x [oy, oy + (cols - 1) hs] only, and
 *   G = {z <= 0}  u  {(x, y) on the grid and z <= H(x, y)}
 * (without a heightfield, the half-space alone).  Then
 *   dist[e, f, k] = inf {t in [0, max_range] : x(t) in G},
 * and max_range exactly when there is no such t (a miss): the ray hit
 * something iff dist < max_range.  normals[e, f, k] is
 *   e_z                       when the half-space z <= 0 is entered first
 *   the triangle's unit       when the terrain solid is entered through a
 *   normal (ground_at's)      triangle
 *   (+-1, 0, 0), (0, +-1, 0)  at the grid's border the surface drops to the
 *                             plane: a ray that enters the terrain solid
 *                             through that vertical face reports the face's
 *                             outward normal; the x face wins at a corner
 *   ground_at's normal at     for a ray that starts inside G (dist = 0)
 *   the start's (x, y)
 *   (0, 0, 0)                 on a miss
 * A ray with a zero or non-finite direction or start, or cast from a
 * non-finite state, reads a miss.  (Finite input so large that the world ray
 * overflows fp32 -- coordinates near 1e38 -- is not promised a miss; the call
 * stays memory-safe and bounded.)  Hits on the robot's own links, on other envs
 * and on the tyres are not modelled.
 *
 * The link poses are formed relative to the root link's origin and the root
 * position is added last, as in tg_height_scan; p_f agrees with
 * tg_rigid_body_states to rounding.  Envs do not interact: an env's results do
 * not depend on the other envs' states.  The walk over the heightfield's cells
 * is bounded by rows + cols + 4 cells per ray whatever the input.
 *
 * TG_ERR_ARG (message "tg_ray_cast: ...") with nothing launched, in this
 * order: null frames, rays or params, dist and normals both NULL, num_frames
 * outside 1..TG_RAY_MAX_FRAMES, num_rays outside 1..TG_RAY_MAX_RAYS, a
 * negative link, a non-finite offset, align outside {0, 1, 2}, a max_range
 * that is not finite and > 0, a null sim, a link >= L: what needs no sim
 * first, then the sim, then the links.  Every model, run-time (tg_model_jit)
 * ones included. */
#define TG_RAY_MAX_FRAMES 8
#define TG_RAY_MAX_RAYS   4096          /* per frame */
#define TG_RAY_LINK  0   /* pattern in the link's own axes (full 3-D rotation R_l) */
#define TG_RAY_YAW   1   /* pattern turned by the link's heading Rz(psi), tg_height_scan's rule */
#define TG_RAY_WORLD 2   /* pattern in world axes */
typedef struct tg_ray_params {   /* HOST, read during the call */
    int32_t align;
    float max_range;
} tg_ray_params;                 /* 8 bytes */
int tg_ray_cast(tg_sim *sim, const tg_contact_frame *frames /* HOST */, int32_t num_frames,
                const float *rays /* [R, 6] device */, int32_t num_rays,
                const tg_ray_params *params /* HOST */,
                float *dist /* [N, F, R] device or NULL */,
                float *normals /* [N, F, R, 3] device or NULL */);
/* Self-collision sensing in one kernel: the signed distances between pairs of
 * capsules fixed to the robot's own links, optionally their witness points and
 * a per-env summary -- what a policy needs to be kept from crossing its legs
 * or swinging a forearm through the chest.  The step models contact with the
 * ground only; this call is a sensor, there is no contact response between
 * links.  On demand, stream-ordered, from the current root and dof state;
 * nothing of the sim is written and nothing is kept on the host between calls.
 * A NULL output is not touched; every element of every non-NULL output is
 * written.
 *
 * Capsule k on link l has the world axis
 *   x(s) = o_l + R_l (p0 + s (p1 - p0)),   s in [0, 1]
 * (o_l and R_l those of tg_rigid_body_states) and the radius r_k; p0 == p1 is
 * a sphere.  Two capsules on the same link are allowed.  pairs [P, 2] holds
 * indices into capsules; for pair p = (a, b), delta is the least distance
 * between the two axis segments, and
 *   dist[e, p]    = delta - r_a - r_b; a negative value is the penetration
 *                   depth
 *   witness[e, p] = a minimising point on axis a (3), then one on axis b (3),
 *                   in world coordinates; where the minimiser is not unique
 *                   (parallel, overlapping axes) any minimiser may be returned
 *   summary[e]    = [0] the smallest dist over the pairs
 *                   [1] the lowest pair index that attains it, as a float
 *                   [2] the number of pairs with dist < margin
 *                   [3] sum_p max(0, margin - dist_p), the self-collision
 *                       penalty of a reward
 * The link poses are formed relative to the root link's origin and the root
 * position is added last, and only to witness: dist and summary do not depend
 * on where the env stands.  summary is reduced in a fixed order, so it is
 * bit-reproducible from call to call.  Envs do not interact.  The kernel forms
 * no index from device data; the distances of a non-finite state are not
 * specified, the call stays memory-safe.
 *
 * TG_ERR_ARG (message "tg_proximity: ...") with nothing launched, in this
 * order: a null sim, null capsules, pairs or params, num_capsules outside
 * 1..TG_PROX_MAX_CAPSULES, num_pairs outside 1..TG_PROX_MAX_PAIRS, a link
 * outside [0, L), a non-finite end point or radius or a negative radius, a
 * pair index outside [0, C) or a pair of a capsule with itself, a non-finite
 * margin, all three outputs NULL.  Every model, run-time (tg_model_jit) ones
 * included. */
#define TG_PROX_MAX_CAPSULES 32
#define TG_PROX_MAX_PAIRS    256
typedef struct tg_capsule {      /* HOST, read during the call */
    int32_t link;                /* [0, L) */
    float p0[3], p1[3];          /* axis end points in the link frame; p0 == p1: a sphere */
    float radius;                /* >= 0 */
} tg_capsule;                    /* 32 bytes */
typedef struct tg_proximity_params {   /* HOST, read during the call */
    float margin;
} tg_proximity_params;           /* 4 bytes */
int tg_proximity(tg_sim *sim, const tg_capsule *capsules /* HOST */, int32_t num_capsules,
                 const int32_t *pairs /* HOST [P, 2], indices into capsules */, int32_t num_pairs,
                 const tg_proximity_params *params /* HOST */,
                 float *dist /* [N, P] device or NULL */,
                 float *witness /* [N, P, 6] device or NULL */,
                 float *summary /* [N, 4] device or NULL */);
/* Contact forces inside friction cones and sole outlines in one kernel launch:
 * tg_contact_inverse_dynamics with the distribution replaced by one that
 * respects the contact model -- unilateral forces, Coulomb friction, the centre
 * of pressure inside the sole -- so that the joint torques assume only wrenches
 * the ground can supply, and what it cannot supply is reported.  On demand,
 * stream-ordered, computed from the current root and dof state, the sim's
 * current gravity, the env's body mass scales and its TG_PROP_ARMATURE and
 * TG_PROP_EFFORT rows; nothing of the sim is written.  contacts, extents and
 * dofs are HOST memory, read during the call and not retained (they travel to
 * the kernel by value in its arguments).
 *
 * b = H a + h, p_k = o_l + R_l offset_k, c_root, Jp_k, terms, accel, efforts,
 * dofs, num_dofs and accumulate are those of tg_contact_inverse_dynamics.
 * Contact k of K (1..TG_CID_MAX_CONTACTS) is a rectangular patch on link l_k
 * with the four vertices
 *   p_kv = o_l + R_l (offset_k + (+-hx_k, +-hy_k, 0)),  v = 0..3 in the order (+,+), (+,-), (-,-), (-,+),
 * (hx_k, hy_k) = extents[k] >= 0 the half extents in the link's x and y axes;
 * zero extents give a point contact.  The unknowns are the J = 4 K vertex
 * forces f_kv, world axes, acting on the robot, each confined to the friction
 * cone of its contact:
 *   C_k = { f : f.n_k >= 0, |f - (f.n_k) n_k| <= mu_k f.n_k }
 * n_k from normals [N, K, 3] (e.g. tg_height_scan's), normalised in the kernel;
 * a non-finite entry or a vector shorter than 1e-6 gives world z, NULL gives
 * world z.  mu_k from friction [N, K], or the scalar mu where friction is NULL;
 * negative and NaN values are taken as 0, values above 1e6 as 1e6.  With
 * r_kv = p_kv - c_root, G_kv = [1; [r_kv]x] (6 x 3) and W = diag(1, 1, 1,
 * 1/l^2, 1/l^2, 1/l^2), l = moment_arm > 0, the call approaches
 *   minimise  1/2 |b[0:6] - sum G_kv f_kv|^2_W  +  1/2 reg sum_k (1/s_k) sum_v |f_kv|^2   over f_kv in C_k
 * (moments about c_root, as the base rows of b are).  s_k >= 0 is the share
 * (share [N, K]; NULL: all ones; negative and NaN values are taken as 0).  A
 * contact with s_k = 0 is removed: its forces and its wrench are exactly 0.0
 * and the env's other outputs equal those of a call without it.  An env with
 * every s_k = 0 gets tau = b and makes no iterations.  The balance is soft on
 * purpose: when b[0:6] is infeasible the answer is the nearest feasible one and
 * the shortfall is returned in tau[0:6], not hidden.
 *
 * The algorithm is fixed, so that a reference can run the same one: over-relaxed
 * ADMM in scaled form from z = u = 0.  With f the stacked vertex forces, G = [G_kv]
 * (6 x 3 J), P = diag(reg / s_k + rho) and c = G^T W b[0:6], each of iters
 * iterations is
 *   q  = c + rho (z - u)
 *   x  = P^-1 q - P^-1 G^T (W^-1 + G P^-1 G^T)^-1 G P^-1 q     (= (G^T W G + P)^-1 q; one 6 x 6 Cholesky factor per env)
 *   xh = relax x + (1 - relax) z
 *   z  = proj_C(xh + u)      per vertex, with w = xh + u, w_n = w.n, t = w - w_n n:
 *                            w_n >= 0 and |t| <= mu w_n: w;  mu |t| <= -w_n: 0;
 *                            else a (n + mu t / |t|), a = (mu |t| + w_n) / (1 + mu^2)
 *   u  = u + xh - z
 * and the result is z: every returned force lies in its cone by construction,
 * after any number of iterations.  reg = 0.03, rho = 0.6, relax = 1.6 and
 * iters = 64 are the values the Python binding passes (DESIGN.md 4.2 has
 * their provenance).
 *
 * forces[e, k, v] = f_kv.  wrench[e, k] = (sum_v f_kv, sum_v (p_kv - p_k) x
 * f_kv): force and moment about p_k, the convention of
 * tg_contact_inverse_dynamics and of the force sensor tensor.  tau[6 + d] =
 * b[6 + d] - sum_k Jp_k[:, 6 + d]^T wrench_k; tau[0:6] = b[0:6] - sum G_kv
 * f_kv is the wrench the ground cannot supply, the feasibility signal.  info[e]
 * = (|tau[0:3]|, |tau[3:6]|, max |x - z| over the components of every vertex in
 * the last iteration, the number of vertices with f.n > 0).  efforts as in
 * tg_contact_inverse_dynamics.  Every element of every non-NULL output is
 * written; with fix_base the full layout is written too.  All lever arms are
 * formed relative to the root link's origin: the result is bit-identical
 * wherever the env sits on the grid.
 *
 * TG_ERR_ARG (message "tg_contact_qp: ...", nothing launched) for a null sim,
 * null contacts, null extents, num_contacts outside 1..TG_CID_MAX_CONTACTS, a
 * link outside [0, L), a link listed twice, an extent not finite or < 0, mu not
 * finite or < 0, moment_arm not finite or <= 0, reg or rho not finite or <= 0,
 * relax outside (0, 2), iters outside 1..TG_QP_MAX_ITERS, tau, wrench, forces,
 * info and efforts all NULL, and every argument error of tg_inverse_dynamics
 * on the arguments the two share.  A rejected call launches nothing.  Every
 * model, run-time (tg_model_jit) ones included. */
#define TG_QP_MAX_ITERS 256
int tg_contact_qp(tg_sim *sim, const tg_contact_frame *contacts /* HOST */, int32_t num_contacts,
                  const float *extents /* HOST [K][2] */,
                  const float *normals /* [N, K, 3] device or NULL (= world z) */,
                  const float *friction /* [N, K] device or NULL (= mu) */, float mu,
                  const float *share /* [N, K] device or NULL (= 1) */,
                  float moment_arm, float reg, float rho, float relax, int32_t iters,
                  int32_t terms, const float *accel /* [N, 6+D] or NULL */,
                  float *tau /* [N, 6+D] device or NULL */,
                  float *wrench /* [N, K, 6] device or NULL */,
                  float *forces /* [N, K, 4, 3] device or NULL */,
                  float *info /* [N, 4] device or NULL */,
                  float *efforts /* [N, D] device or NULL */,
                  const int32_t *dofs /* HOST */, int32_t num_dofs, int32_t accumulate);
/* fetch_results(sim, True): waits for the sim stream.  Also reports (once, as
 * TG_ERR_STATE) a state error a kernel raised since the last call: a locked
 * DOF whose [lower, upper] window was widened beyond TG_LOCK_WINDOW_MAX. */
int tg_sync(tg_sim *sim);
const char *tg_last_error(void);
uint64_t tg_compiled_model_hashes(uint64_t *out, int32_t cap); /* returns count */
/* gym.load_asset of a model that is not compiled in (gogoro_new.py:198-213
 * loads its URDF at run time): compile the articulation kernels for it with
 * hipRTC (gfx950) and register them under model_hash, after which
 * tg_sim_create accepts a tg_model_desc with that hash.  model_source is the
 * model's constexpr table text as thormang_isaacgym_amd/model/codegen.py emits
 * it (one `struct <struct_name> {...}`; the Python host parses the URDF and
 * produces both it and the tg_model_desc).  include_dir: the kernel headers
 * (NULL: the csrc/ directory beside libtgsim.so); cache_dir: where code objects
 * are cached by hash and source digest (NULL: no cache).  A no-op for a
 * compiled-in hash or one already registered in this process. */
int tg_model_jit(uint64_t model_hash, const char *struct_name, const char *model_source, const char *include_dir,
                 const char *cache_dir);

/* gym.load_asset of a URDF without a Python host (gogoro_new.py:198-213, the
 * locked joints of :257-262): csrc/model_load.cpp parses the file (links
 * depth-first from the root, children in joint-declaration order, DOFs = the
 * non-fixed joints in that order, fixed and `locked_joints` merged into rigid
 * groups, collision boxes / spheres, a mesh collision as the torus fitted to
 * its OBJ profile when `mesh_root` names the mesh directory) and builds the
 * tg_model_desc and the specialisation's constexpr source exactly as the
 * Python host (model/urdf.py, abi.model_arrays, model/codegen.py) does.
 * tg_model_parse stops there (no device needed); tg_model_load then runs
 * tg_model_jit for it (a no-op for a compiled-in model).  `name`: the model
 * name (NULL: the file's stem).  The desc arrays live in the tg_model until
 * tg_model_free; errors: tg_model_last_error(). */
typedef struct tg_model tg_model;
int tg_model_parse(const char *urdf_path, const char *name, const char *const *locked_joints, int32_t num_locked,
                   const char *mesh_root, tg_model **out);
int tg_model_load(const char *urdf_path, const char *name, const char *const *locked_joints, int32_t num_locked,
                  const char *mesh_root, const char *cache_dir, tg_model **out);
int tg_model_get_desc(const tg_model *model, tg_model_desc *desc);   /* pointers into the model */
const char *tg_model_dof_name(const tg_model *model, int32_t dof);   /* gym.get_asset_dof_names order */
const char *tg_model_link_name(const tg_model *model, int32_t link); /* gym.get_asset_rigid_body_names */
/* gym.get_asset_dof_properties' URDF part (lower, upper, effort, velocity;
 * +-3.4e38 for an unlimited joint) */
int tg_model_dof_limits(const tg_model *model, int32_t dof, float *lower, float *upper, float *effort,
                        float *velocity);
const char *tg_model_source(const tg_model *model);   /* the constexpr traits text (codegen.emit) */
const char *tg_model_last_error(void);
void tg_model_free(tg_model *model);

/* Composite-cache instrumentation (no reference counterpart; tests): copies
 * the per-env composite cache [N, KC] (the group composites and placements
 * the step kernel reads, built from the lock windows and mass scales) to the
 * device buffer out; with recompose != 0 every env is first re-composed from
 * scratch.  Checks the Gogoro epilogue's in-place seat update against a full
 * compose.  The re-compose is the launch a simulate makes for dirty envs,
 * shared-cache check included (compose_kernel, then uniform_check_kernel): it
 * leaves the shared-cache flag describing the blocks it wrote, so the next
 * simulate may skip its own compose whether or not the envs still agree. */
int tg_composite(tg_sim *sim, float *out, int32_t recompose);

/* Random-number instrumentation (no reference counterpart; the task kernels'
 * in-kernel draws replace the reference's torch.rand / torch.randn calls):
 * tg_philox4x32_10 is the library's Philox4x32-10 block function on the host
 * (ctr[4], key[2] -> out[4]; the same code the kernels run), checked against
 * Random123's published known-answer vectors.  tg_rng_fill runs it on the
 * device for blocks i = 0..n-1 with counter (i, counter lo, counter hi, 0) and
 * key = seed: kind 0 writes the 4 raw 32-bit words per block (out holds 4n
 * words), kind 1 the 4 uniforms u01(word) in [0, 1), kind 2 the 2 normals
 * gauss(w0, w1), gauss(w2, w3) per block (out holds 2n floats). */
void tg_philox4x32_10(const uint32_t *ctr, const uint32_t *key, uint32_t *out);
int tg_rng_fill(tg_sim *sim, int32_t kind, uint64_t seed, uint64_t counter, float *out, int32_t n);

/* Debug instrumentation (no reference counterpart): fills the LDS of every CU
 * with a 32-bit pattern (a NaN, say) through a dummy launch on the sim's
 * stream.  LDS is not cleared between kernels, so a later step that read LDS
 * it had not written would see the pattern: the stale-LDS tests step two
 * identical envs, one with a fill before every step, and require bit-identical
 * results. */
int tg_debug_fill_lds(tg_sim *sim, uint32_t pattern);

/* Launch-statistics instrumentation (no reference counterpart; tests): the
 * host counters of the launches tg_simulate and the task steps made or skipped
 * since the sim was created -- out[0] full compose launches (every dirty env),
 * out[1] list compose launches (the last fused epilogue's resets), out[2]
 * simulates that skipped the compose launch, out[3] launches of the
 * rigid-body force reduction on its own (a pending
 * tg_apply_rigid_body_force_tensors while the compose is skipped or a list
 * compose), out[4] pending force tensors reduced inside a full compose,
 * out[5] fused task-step launches that were declined (the caller then took its
 * general path).  Plain integers read on the host: no device work, and nothing
 * about what is launched depends on them.  The call-sequence tests use them
 * to show that the cached path under test was really taken. */
int tg_debug_launch_stats(tg_sim *sim, int64_t out[6]);

/* Benchmark instrumentation (no reference counterpart): with period > 0,
 * tg_simulate brackets every period-th articulation step kernel launch with HIP
 * events on the sim stream (an event pair serialises the queue for ~5 us each
 * side, so sampling keeps the instrumented run's throughput honest); with
 * period = -W < 0 it brackets windows of W consecutive step-kernel launches
 * with one pair (no event between the kernels it times; a window another
 * launch of the library falls into is dropped); 0 turns timing off.
 * tg_read_kernel_timing waits for the recorded launches and returns (and
 * resets) the summed kernel time and the timed launch count. */
int tg_set_kernel_timing(tg_sim *sim, int32_t period);
int tg_read_kernel_timing(tg_sim *sim, double *total_ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
