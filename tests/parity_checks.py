"""Step-level parity checks shared by the CPU tier (kernel sources compiled for the host) and the GPU tier (the real
HIP library).  Every check feeds the device path and the oracle IDENTICAL inputs and compares one stage of the hot
path: exact term values, convexified rows / reference-layout CSC, one Model::optimize(), and the SQP state machine.

Why step-level: BasicTrustRegionSQP is discontinuous in its inputs (accept/reject, polish success, the 1e-7
cleanup threshold, the byte-prefix sparsity test that gates OSQP warm starts).  The oracle itself, compiled with vs
without FMA contraction, ends up to 3e-2 rad apart on config 1 with different QP counts, so
end-to-end trajectories are compared statistically, and the bit-exact / 1e-5 bars apply per stage.
"""
import numpy as np

from trajopt_amd import abi, configs

TOL_TRAJ = 1e-5      # rad — north_star tolerance for joint trajectories / QP primal solutions

# configuration ids of cfg() below: every id runs the stage checks on both tiers; MINI_CIDS also the whole SQP
MINI_CIDS = [9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44]
STAGE_CIDS = [0, 1, 2, 3] + MINI_CIDS


def convex_hull_triangles(points):
    """triangles [nt][3][3] of the convex hull of `points`, counter-clockwise seen from outside (scipy's Qhull facets re-oriented)"""
    from scipy.spatial import ConvexHull
    pts = np.asarray(points, dtype=np.float64)
    hull = ConvexHull(pts)
    mid = pts[hull.vertices].mean(axis=0)
    tris = []
    for simplex in hull.simplices:
        a, b, c = pts[simplex]
        if np.dot(np.cross(b - a, c - a), a - mid) < 0:
            b, c = c, b
        tris.append([a, b, c])
    return np.asarray(tris)


def cfg(cid, T=None):
    """config id -> (pci, start, goal); shared by the CPU (host build) and GPU tiers so both run the same problems"""
    if cid == 9:   # shape-coverage problem: 4-DOF, 14 waypoints (configs.config_mini)
        return configs.config_mini() if T is None else configs.config_mini(T)
    if cid == 10:  # the same with JointPosEqCost + JointPosIneqCost terms
        return configs.config_mini(with_pos_costs=True)
    if cid == 11:  # collision as a constraint (CollisionConstraint per step)
        return configs.config_mini(collision_cnt=True)
    if cid == 13:  # 10-DOF chain: outside the dense fast path -> generic block-chain path of the kernels
        return configs.config_wide()
    if cid == 14:  # CollisionTermInfo::fixed_steps independent of BasicInfo::fixed_timesteps: contacts AT the fixed
        return configs.config_mini(collision_fixed_steps=(5,))   # waypoint 0 (constant rows), none at waypoint 5
    if cid == 15:  # no row slot at all: a joint-velocity cost and nothing else (R = 0, the QP is the box-constrained objective)
        from trajopt_amd.problem import BasicInfo, JointVelTermInfo, ProblemConstructionInfo
        rob = configs.mini_arm()
        rob.link_spheres = []
        pci = ProblemConstructionInfo(rob, BasicInfo(n_steps=6 if T is None else T))
        pci.cost_infos.append(JointVelTermInfo(coeffs=[1.0, 2.0, 0.5, 1.5], targets=[0.0] * 4, first_step=0, last_step=pci.basic_info.n_steps - 1))
        return pci, configs.MINI_START, configs.MINI_GOAL
    if cid in (16, 17, 18, 19):
        # segment collision evaluators (pair rows, dense coupling blocks): 16 LVS_DISCRETE cost, 17 LVS_CONTINUOUS (cast) cost,
        # 18 LVS_CONTINUOUS constraint, 19 CONTINUOUS cost whose segments are never split (lvs larger than any step)
        from trajopt_amd.problem import CollisionTermInfo
        pci, s, g = configs.config_mini(collision_cnt=(cid == 18)) if T is None else configs.config_mini(T, collision_cnt=(cid == 18))
        for ti in pci.cost_infos + pci.cnt_infos:
            if isinstance(ti, CollisionTermInfo):
                ti.evaluator_type = {16: 2, 17: 4, 18: 4, 19: 3}[cid]
                ti.longest_valid_segment_length = 10.0 if cid == 19 else 0.12
                ti.max_substates = 2 if cid == 19 else 4
        return pci, s, g
    if cid == 25:
        # two segment collision terms with DIFFERENT max_substates (every row slot carries its term's capacity): an LVS_DISCRETE
        # cost that never splits its segments (capacity 2) next to an LVS_CONTINUOUS constraint with capacity 5
        from trajopt_amd.problem import CollisionTermInfo
        pci, s, g = configs.config_mini() if T is None else configs.config_mini(T)
        n = pci.basic_info.n_steps
        for ti in pci.cost_infos:
            if isinstance(ti, CollisionTermInfo):
                ti.evaluator_type, ti.longest_valid_segment_length, ti.max_substates = 2, 0.12, 2
        pci.cnt_infos.insert(0, CollisionTermInfo(first_step=0, last_step=n - 1, dist_pen=0.02, coeff=3.0, safety_margin_buffer=0.2,
                                                  is_constraint=True, fixed_steps=[0], evaluator_type=4,
                                                  longest_valid_segment_length=0.1, max_substates=5))
        return pci, s, g
    if cid in (20, 21, 22):
        # CAPSULE obstacles (include/tmx_geom.h): 20 single-time-step cost, 21 LVS_CONTINUOUS (swept link sphere vs capsule =
        # closest points of two segments) cost, 22 LVS_DISCRETE constraint; one capsule across the path + the original sphere
        from trajopt_amd.problem import CollisionTermInfo
        pci, s, g = configs.config_mini(collision_cnt=(cid == 22)) if T is None else configs.config_mini(T, collision_cnt=(cid == 22))
        (c0, r0) = pci.obstacles[0]
        pci.obstacles = [((c0[0] - 0.25, c0[1] - 0.1, c0[2] + 0.05), 0.06, (0.5, 0.15, -0.1)), (c0, r0)]
        for ti in pci.cost_infos + pci.cnt_infos:
            if isinstance(ti, CollisionTermInfo) and cid != 20:
                ti.evaluator_type = 4 if cid == 21 else 2
                ti.longest_valid_segment_length = 0.12
                ti.max_substates = 4
        return pci, s, g
    if cid in (23, 24):
        # CartVelTermInfo (rows on two waypoints with analytic Jacobians): 23 INEQ constraint, 24 ABS cost; the limit is tighter
        # than the straight-line tool motion per step, so the rows are active
        from trajopt_amd.problem import CartVelTermInfo
        pci, s, g = configs.config_mini(with_joint_band=False) if T is None else configs.config_mini(T, with_joint_band=False)
        n = pci.basic_info.n_steps
        ti = CartVelTermInfo(first_step=1, last_step=n - 2, max_displacement=0.07, is_constraint=(cid == 23))
        (pci.cnt_infos if cid == 23 else pci.cost_infos).append(ti)
        return pci, s, g
    if cid in (54, 55, 56):
        # round 6: the BUILT-IN kinematic function terms inside a time-parameterised problem (refused until round 5).  Base = config 50
        # (velocity limits with time as INEQ constraints + TotalTime cost, 4-DOF test arm: fewer joints than Jacobian rows, so a zero
        # time column in the decomposed Jacobian would make the smallest singular value 0).  54: AvoidSingularity ABS cost over the
        # problem's joint group; 55: the DynamicCartPose ABS cost of 43 (tolerance band) in place of the static via point; 56: the static
        # via point with the tolerance band of 42 + AvoidSingularity over the joint subset 1 .. 3 as INEQ constraint
        from trajopt_amd.problem import AvoidSingularityTermInfo, CartPoseTermInfo, DynamicCartPoseTermInfo
        pci, s, g = cfg(50, T)
        D, n = pci.robot.n_dof, pci.basic_info.n_steps
        if cid == 54:
            pci.cost_infos.append(AvoidSingularityTermInfo(link=D - 1, first_step=1, last_step=n - 2, coeffs=[2.0], lambda_=0.1, name="sing"))
        elif cid == 55:
            pci.cnt_infos = [ti for ti in pci.cnt_infos if not isinstance(ti, CartPoseTermInfo)]
            qv = 0.5 * (s + g) + np.array([0.1, -0.15, 0.2, 0.1])
            off = (np.linalg.inv(pci.robot.fk_links(qv)[1]) @ pci.robot.fk_tool(qv))[:3, :]
            pci.cost_infos.insert(0, DynamicCartPoseTermInfo(timestep=n // 2, target_link=1, target_frame_offset=off, pos_coeffs=(2, 1, 1.5),
                                                             rot_coeffs=(0.5, 0.25, 1.0), is_constraint=False, lower_tolerance=[-0.03, -0.02, -0.01, -0.2, -0.1, -0.05],
                                                             upper_tolerance=[0.02, 0.03, 0.04, 0.1, 0.2, 0.3]))
        else:
            for ti in pci.cnt_infos:
                if isinstance(ti, CartPoseTermInfo):
                    ti.lower_tolerance = [-0.02, -0.01, -0.03, 0, 0, 0]
                    ti.upper_tolerance = [0.01, 0.02, 0.0, 0, 0, 0]
            pci.cnt_infos.append(AvoidSingularityTermInfo(link=3, first_step=1, last_step=n - 2, coeffs=[1.0], lambda_=0.05, subset_first=1,
                                                          is_constraint=True, name="sing"))
        return pci, s, g
    if cid in (48, 49, 50, 51, 52, 53):
        # TIME-PARAMETERISED problems (BasicInfo::use_time: one 1/dt variable per waypoint; problem_description.cpp:1244-1325, :1852-1890)
        # on the 4-DOF test arm (53: glass_upright): 48 JointVel-with-time SQUARED cost + TotalTime HINGE cost; 49 velocity limits as a
        # HINGE cost + TotalTime INEQ constraint; 50 the time-optimal shape: velocity limits as INEQ constraints, TotalTime cost; 51 velocity
        # EQ constraints on two segments + TotalTime SQUARED cost (limit 0); 52 = 48 without a TotalTime term (time enters through the
        # velocity cost only); 53 ROWS ONLY - velocity limits as INEQ constraints and a HINGE velocity cost, no TotalTime: the QP stays a
        # block chain with pair rows and runs on the structured solvers (no dense engine, no size limit)
        from trajopt_amd.problem import JointVelTermInfo, TotalTimeTermInfo
        pci, s, g = configs.config_mini() if T is None else configs.config_mini(T)
        D, n = pci.robot.n_dof, pci.basic_info.n_steps
        pci.basic_info.use_time = True
        pci.basic_info.dt_lower_lim, pci.basic_info.dt_upper_lim = 0.4, 6.0
        plain = pci.cost_infos[0]
        assert isinstance(plain, JointVelTermInfo)
        if cid in (48, 52):
            pci.cost_infos[0] = JointVelTermInfo(coeffs=[1.0, 2.0, 0.5, 1.5], targets=[0.0] * D, first_step=0, last_step=n - 1, use_time=True, name="vel_t")
            if cid == 48:
                pci.cost_infos.append(TotalTimeTermInfo(coeff=0.3, limit=0.5 * (n - 1), name="total_time"))
        elif cid == 49:
            pci.cost_infos.insert(1, JointVelTermInfo(coeffs=[2.0, 1.0, 3.0, 1.5], targets=[0.0] * D, first_step=1, last_step=n - 2, use_time=True,
                                                      upper_tols=[0.08, 0.1, 0.06, 0.12], lower_tols=[-0.08, -0.1, -0.06, -0.12], name="vel_lim"))
            pci.cnt_infos.insert(0, TotalTimeTermInfo(coeff=1.0, limit=0.7 * (n - 1), is_constraint=True, name="total_time"))
        elif cid == 53:
            pci.cnt_infos.insert(0, JointVelTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=n - 1, use_time=True, is_constraint=True,
                                                     upper_tols=[0.2] * D, lower_tols=[-0.2] * D, name="vel_lim"))
            pci.cost_infos.insert(1, JointVelTermInfo(coeffs=[2.0, 1.0, 3.0, 1.5], targets=[0.0] * D, first_step=1, last_step=n - 2, use_time=True,
                                                      upper_tols=[0.08, 0.1, 0.06, 0.12], lower_tols=[-0.08, -0.1, -0.06, -0.12], name="vel_soft"))
        elif cid == 50:
            pci.cnt_infos.insert(0, JointVelTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=n - 1, use_time=True, is_constraint=True,
                                                     upper_tols=[0.25] * D, lower_tols=[-0.25] * D, name="vel_lim"))
            pci.cost_infos.append(TotalTimeTermInfo(coeff=2.0, limit=0.2 * (n - 1), name="total_time"))
        else:
            pci.cnt_infos.insert(0, JointVelTermInfo(coeffs=[1.0, 0.5, 2.0, 1.0], targets=list((g - s) / (n - 1)), first_step=2, last_step=4, use_time=True,
                                                     is_constraint=True, name="vel_eq"))
            pci.cost_infos.append(TotalTimeTermInfo(coeff=0.01, limit=0.0, name="total_time"))
        return pci, s, g
    if cid in (45, 46, 47):
        # CONVEX-HULL LINKS (include/tmx_gjk.h): the last two link spheres of the test arm become a box hull (rounded by 1 cm) and a
        # wedge hull; 45 single-time-step cost against the sphere + a box obstacle, 46 LVS_CONTINUOUS (cast: hulls swept over the
        # sub-segments) cost, 47 LVS_DISCRETE constraint with a convex-mesh obstacle on top
        from trajopt_amd.problem import CollisionTermInfo
        pci, s, g = configs.config_mini(collision_cnt=(cid == 47)) if T is None else configs.config_mini(T, collision_cnt=(cid == 47))
        rob = pci.robot
        box = np.array([[sx * 0.09, sy * 0.04, sz * 0.03] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) + np.array([0.15, 0.0, 0.0])
        wedge = np.array([[0.02, -0.03, -0.03], [0.02, 0.03, -0.03], [0.02, 0.0, 0.04], [0.2, -0.02, -0.02], [0.2, 0.02, -0.02], [0.2, 0.0, 0.02]])
        rob.link_spheres = [rob.link_spheres[0], (2, (0.0, 0.0, 0.0), 0.01, ("hull", box)), (3, (0.0, 0.0, 0.0), 0.0, ("hull", wedge))]
        (c0, r0) = pci.obstacles[0]
        pci.obstacles = [(c0, r0), ((c0[0] - 0.2, c0[1] + 0.1, c0[2] + 0.12), 0.01, ("box", (0.06, 0.1, 0.05), None))]
        if cid == 47:
            from scipy.spatial import ConvexHull
            V = np.array([[0.0, 0.0, 0.0], [0.12, 0.0, 0.0], [0.0, 0.12, 0.0], [0.0, 0.0, 0.12], [0.1, 0.1, 0.1]]) + np.array([c0[0] + 0.1, c0[1] - 0.25, c0[2] + 0.15])
            H = ConvexHull(V)
            tris = []
            for simp, eq in zip(H.simplices, H.equations):
                a, b, c = V[simp]
                if np.cross(b - a, c - a) @ eq[:3] < 0:
                    b, c = c, b
                tris.append([a, b, c])
            pci.obstacles.append(((0.0, 0.0, 0.0), 0.0, ("mesh", np.array(tris))))
        for ti in pci.cost_infos + pci.cnt_infos:
            if isinstance(ti, CollisionTermInfo) and cid != 45:
                ti.evaluator_type = 4 if cid == 46 else 2
                ti.longest_valid_segment_length = 0.12
                ti.max_substates = 4
        return pci, s, g
    if cid == 44:
        # AvoidSingularity over a joint SUBSET (subset_kin_): joints 1 .. 6 of the PR2 arm on an 8-waypoint glass_upright, ABS cost
        from trajopt_amd.problem import AvoidSingularityTermInfo
        pci, s, g = configs.config1(8 if T is None else T)
        n = pci.basic_info.n_steps
        pci.cost_infos.append(AvoidSingularityTermInfo(link=6, first_step=1, last_step=n - 2, coeffs=[1.5], lambda_=0.1, subset_first=1, name="sing"))
        return pci, s, g
    if cid in (38, 39):
        # AvoidSingularityTermInfo (built-in kinematic function of the function-term machinery, dense QP engine): 38 ABS cost on the
        # 4-DOF test arm (fewer joints than Jacobian rows: the singular triplet comes from J'J), 39 INEQ constraint on a 10-waypoint
        # glass_upright (7 joints: from JJ')
        from trajopt_amd.problem import AvoidSingularityTermInfo
        if cid == 38:
            pci, s, g = configs.config_mini() if T is None else configs.config_mini(T)
        else:
            pci, s, g = configs.config1(10 if T is None else T)
        D, n = pci.robot.n_dof, pci.basic_info.n_steps
        ti = AvoidSingularityTermInfo(link=D - 1, first_step=1, last_step=n - 2, coeffs=[2.0 if cid == 38 else 1.0], lambda_=0.1 if cid == 38 else 0.05,
                                      is_constraint=(cid == 39), name="sing")
        (pci.cnt_infos if cid == 39 else pci.cost_infos).append(ti)
        return pci, s, g
    if cid in (42, 43):
        # pose terms with a TOLERANCE BAND (CartPoseTermInfo / DynamicCartPoseTermInfo lower_tolerance / upper_tolerance): 42 the static via
        # point of the 4-DOF test arm with a band that holds part of the seeds' error, 43 the dynamic ABS cost of 41 with a band
        from trajopt_amd.problem import CartPoseTermInfo, DynamicCartPoseTermInfo
        if cid == 42:
            pci, s, g = configs.config_mini() if T is None else configs.config_mini(T)
            for ti in pci.cnt_infos:
                if isinstance(ti, CartPoseTermInfo):
                    ti.lower_tolerance = [-0.02, -0.01, -0.03, 0, 0, 0]
                    ti.upper_tolerance = [0.01, 0.02, 0.0, 0, 0, 0]
            return pci, s, g
        pci, s, g = cfg(41, T)
        for ti in pci.cost_infos:
            if isinstance(ti, DynamicCartPoseTermInfo):
                ti.lower_tolerance = [-0.03, -0.02, -0.01, -0.2, -0.1, -0.05]
                ti.upper_tolerance = [0.02, 0.03, 0.04, 0.1, 0.2, 0.3]
        return pci, s, g
    if cid in (40, 41):
        # DynamicCartPoseTermInfo (both frames move): the tool relative to link 1 of the 4-DOF test arm at the middle waypoint, in
        # place of the static via point; 40 EQ constraint on the position rows, 41 ABS cost on all six rows
        from trajopt_amd.problem import CartPoseTermInfo, DynamicCartPoseTermInfo
        pci, s, g = configs.config_mini() if T is None else configs.config_mini(T)
        n = pci.basic_info.n_steps
        pci.cnt_infos = [ti for ti in pci.cnt_infos if not isinstance(ti, CartPoseTermInfo)]
        qv = 0.5 * (s + g) + np.array([0.1, -0.15, 0.2, 0.1])
        off = (np.linalg.inv(pci.robot.fk_links(qv)[1]) @ pci.robot.fk_tool(qv))[:3, :]
        ti = DynamicCartPoseTermInfo(timestep=n // 2, target_link=1, target_frame_offset=off, pos_coeffs=(1, 1, 1) if cid == 40 else (2, 1, 1.5),
                                     rot_coeffs=(0, 0, 0) if cid == 40 else (0.5, 0.25, 1.0), is_constraint=(cid == 40))
        (pci.cnt_infos if cid == 40 else pci.cost_infos).insert(0, ti)
        return pci, s, g
    if cid in (36, 37):
        # acceleration + jerk SMOOTHING COSTS alone (banded objective, no rows on 3 - 4 waypoints): the structured solver's banded block
        # factorisation (DevProblem::band), not the dense engine; 36 the 4-DOF test arm, 37 a 12-waypoint glass_upright (config 1)
        from trajopt_amd.problem import JointAccTermInfo, JointJerkTermInfo
        if cid == 36:
            pci, s, g = configs.config_mini() if T is None else configs.config_mini(T)
        else:
            pci, s, g = configs.config1(12 if T is None else T)
        D, n = pci.robot.n_dof, pci.basic_info.n_steps
        pci.cost_infos.append(JointAccTermInfo(coeffs=list(np.linspace(0.5, 2.0, D)), targets=[0.0] * D, first_step=0, last_step=n - 1, name="acc"))
        pci.cost_infos.insert(1, JointJerkTermInfo(coeffs=list(np.linspace(1.5, 0.4, D)), targets=[0.0] * D, first_step=1, last_step=n - 1, name="jerk"))
        return pci, s, g
    if cid in (34, 35):
        # CONVEX-MESH obstacles (tmx_problem_desc::obstacle_mesh / mesh_triangles): the convex hull of 14 points across the path, rounded
        # by 1 cm, next to the original sphere; 34 single-time-step cost, 35 LVS_CONTINUOUS (cast) constraint
        from trajopt_amd.problem import CollisionTermInfo
        pci, s, g = configs.config_mini(collision_cnt=(cid == 35)) if T is None else configs.config_mini(T, collision_cnt=(cid == 35))
        (c0, r0) = pci.obstacles[0]
        pts = np.asarray(c0)[None, :] + np.array([-0.05, 0.02, 0.12])[None, :] + np.random.default_rng(7).uniform(-1, 1, (14, 3)) * np.array([0.14, 0.18, 0.06])
        pci.obstacles = [(tuple(pts.mean(axis=0)), 0.01, ("mesh", convex_hull_triangles(pts))), (c0, r0)]
        for ti in pci.cost_infos + pci.cnt_infos:
            if isinstance(ti, CollisionTermInfo) and cid == 35:
                ti.evaluator_type, ti.longest_valid_segment_length, ti.max_substates = 4, 0.12, 4
        return pci, s, g
    if cid in (31, 32, 33):
        # BOX obstacles (tmx_problem_desc::obstacle_boxes): a rotated, rounded box across the path next to the original sphere;
        # 31 single-time-step cost with sphere links, 32 LVS_CONTINUOUS (cast: swept link spheres against the box by the golden-section
        # search on the box's signed distance) cost, 33 capsule links + LVS_DISCRETE constraint
        from trajopt_amd.problem import CollisionTermInfo, rot_axis
        pci, s, g = configs.config_mini(collision_cnt=(cid == 33)) if T is None else configs.config_mini(T, collision_cnt=(cid == 33))
        (c0, r0) = pci.obstacles[0]
        Rb = rot_axis(np.array([0.0, 0.0, 1.0]), 0.4) @ rot_axis(np.array([1.0, 0.0, 0.0]), 0.25)
        pci.obstacles = [((c0[0] - 0.05, c0[1] + 0.02, c0[2] + 0.1), 0.02, ("box", (0.12, 0.2, 0.05), Rb)), (c0, r0)]
        if cid == 33:
            pci.robot.link_spheres = [(1, (0.08, 0.0, 0.0), 0.06, (0.2, 0.0, 0.0)), (2, (0.06, 0.0, 0.0), 0.05, (0.18, 0.0, 0.01)), (3, (0.1, 0.0, 0.0), 0.05)]
        for ti in pci.cost_infos + pci.cnt_infos:
            if isinstance(ti, CollisionTermInfo) and cid != 31:
                ti.evaluator_type = 4 if cid == 32 else 2
                ti.longest_valid_segment_length = 0.12
                ti.max_substates = 4
        return pci, s, g
    if cid in (29, 30):
        # CAPSULE LINKS (tmx_problem_desc::link_sphere_axes): the three link primitives of the test arm become capsules along their
        # links; 29 single-time-step cost against the sphere + a capsule obstacle, 30 LVS_DISCRETE constraint
        from trajopt_amd.problem import CollisionTermInfo
        pci, s, g = configs.config_mini(collision_cnt=(cid == 30)) if T is None else configs.config_mini(T, collision_cnt=(cid == 30))
        rob = pci.robot
        rob.link_spheres = [(1, (0.08, 0.0, 0.0), 0.06, (0.2, 0.0, 0.0)), (2, (0.06, 0.0, 0.0), 0.05, (0.18, 0.0, 0.01)), (3, (0.1, 0.0, 0.0), 0.05)]
        (c0, r0) = pci.obstacles[0]
        pci.obstacles = [((c0[0] - 0.25, c0[1] - 0.1, c0[2] + 0.05), 0.05, (0.5, 0.15, -0.1)), (c0, r0)]
        if cid == 30:
            for ti in pci.cost_infos + pci.cnt_infos:
                if isinstance(ti, CollisionTermInfo):
                    ti.evaluator_type, ti.longest_valid_segment_length, ti.max_substates = 2, 0.12, 4
        return pci, s, g
    if cid in (26, 27, 28):
        # JointAcc / JointJerk terms (rows on 3 / 4 waypoints, banded objective -> dense QP engine) next to the mini arm's collision
        # cost, via-point constraint and joint band: 26 acceleration smoothing cost + acceleration limits (INEQ constraint),
        # 27 jerk smoothing cost + a jerk EQ constraint over the first steps + jerk hinge cost, 28 all three difference orders
        # (velocity EQ constraint, acceleration hinge cost, jerk limits) interleaved in one problem
        from trajopt_amd.problem import JointAccTermInfo, JointJerkTermInfo, JointVelTermInfo
        pci, s, g = configs.config_mini() if T is None else configs.config_mini(T)
        n, D = pci.basic_info.n_steps, 4
        if cid == 26:
            pci.cost_infos.append(JointAccTermInfo(coeffs=[2.0, 1.0, 0.5, 1.5], targets=[0.0] * D, first_step=0, last_step=n - 1, name="acc_smooth"))
            pci.cnt_infos.insert(0, JointAccTermInfo(coeffs=[1.0, 2.0, 1.0, 0.5], targets=[0.0] * D, first_step=1, last_step=n - 2,
                                                     upper_tols=[0.05, 0.04, 0.06, 0.05], lower_tols=[-0.05, -0.03, -0.06, -0.04],
                                                     is_constraint=True, name="acc_limits"))
        elif cid == 27:
            pci.cost_infos.insert(1, JointJerkTermInfo(coeffs=[1.0, 0.5, 2.0, 1.0], targets=[0.0] * D, first_step=0, last_step=n - 1, name="jerk_smooth"))
            pci.cost_infos.append(JointJerkTermInfo(coeffs=[3.0, 2.0, 1.0, 1.0], targets=[0.01, 0.0, -0.01, 0.0], first_step=2, last_step=n - 2,
                                                    upper_tols=[0.02] * D, lower_tols=[-0.02, -0.01, -0.02, -0.03], name="jerk_hinge"))
            pci.cnt_infos.append(JointJerkTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=4, is_constraint=True, name="jerk_eq"))
        else:
            pci.cnt_infos.append(JointVelTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=n - 2, last_step=n - 1, is_constraint=True,
                                                  name="stop"))
            pci.cost_infos.append(JointAccTermInfo(coeffs=[2.0, 2.0, 1.0, 1.0], targets=[0.0] * D, first_step=0, last_step=n - 1,
                                                   upper_tols=[0.03] * D, lower_tols=[-0.03] * D, name="acc_hinge"))
            pci.cnt_infos.insert(0, JointJerkTermInfo(coeffs=[1.0] * D, targets=[0.0] * D, first_step=0, last_step=n - 1,
                                                      upper_tols=[0.08] * D, lower_tols=[-0.08] * D, is_constraint=True, name="jerk_limits"))
            pci.cost_infos.append(JointJerkTermInfo(coeffs=[0.5] * D, targets=[0.0] * D, first_step=0, last_step=n - 1, name="jerk_smooth"))
        return pci, s, g
    if cid == 12:  # BasicInfo::fixed_dofs: the wrist joint keeps its seed value at every step
        return configs.config_mini(with_joint_band=False, fixed_dofs=[3])
    if cid == 2:   # puzzle_piece: 300 waypoints, the QP workspace lives in HBM on the device (generic block-chain path)
        return configs.config2() if T is None else configs.config2(T)
    if cid == 3:   # car_seat: 10-DOF, 50 waypoints, 20 obstacles, LVS_CONTINUOUS collision (pair rows; workspace in HBM)
        return configs.config3() if T is None else configs.config3(T)
    if cid == 0:
        pci, s, g = configs.config0() if T is None else configs.config0(T)
    else:
        pci, s, g = configs.config1() if T is None else configs.config1(T)
    return pci, s, g


def make_ctx_inputs(ctx, pci, x0, sqp=None, osqp=None):
    desc = pci.to_desc()
    ctx.upload(desc, sqp or abi.default_sqp_params(), osqp or abi.default_osqp_settings())
    ctx.set_x0(x0)
    return desc


def check_evaluate(ctx, orc, desc, x0, tol):
    cv, vv = ctx.evaluate()
    for b in range(x0.shape[0]):
        ocv, ovv = orc.evaluate(desc, x0[b], x0[b])
        assert cv[b].shape == ocv.shape and vv[b].shape == ovv.shape
        assert np.abs(cv[b] - ocv).max(initial=0.0) <= tol, "cost values differ"
        assert np.abs(vv[b] - ovv).max(initial=0.0) <= tol, "constraint violations differ"


def check_first_qp_structure(ctx, orc, desc, x0, b, val_tol):
    """convexify at x0[b] and compare the QP handed to osqp_setup: integer CSC arrays bit-exact (ALWAYS: device and oracle
    share include/tmx_detmath.h, so even the mathematically-zero 1e-17 entries the reference keeps - solver_utils.cpp:111-144
    drops exact zeros only - are the same on both sides), values to val_tol."""
    ctx.convexify()
    e = ctx.export_csc(b)
    q = orc.first_qp(desc, x0[b])
    assert (e["n"], e["m"]) == (q["n"], q["m"])
    for k in ("P_p", "P_i", "A_p", "A_i"):
        assert np.array_equal(e[k], q[k]), f"{k}: integer CSC arrays must be bit-exact"
    for k in ("A_x", "P_x", "q", "l", "u"):
        assert np.abs(e[k] - q[k]).max(initial=0.0) <= val_tol, f"{k} differs by {np.abs(e[k] - q[k]).max()}"
    return q


def csc_dense_ops(qp):
    """(P symmetric from the upper triangle, A) as scipy CSC matrices of an exported / oracle QP dict"""
    import scipy.sparse as sp
    n, m = qp["n"], qp["m"]
    Pu = sp.csc_matrix((qp["P_x"], qp["P_i"], qp["P_p"]), shape=(n, n))
    P = Pu + sp.triu(Pu, 1).T
    A = sp.csc_matrix((qp["A_x"], qp["A_i"], qp["A_p"]), shape=(m, n))
    return P, A


def kkt_certificate(qp, x, y):
    """Oracle-INDEPENDENT optimality certificate of (x, y) for  min 1/2 x'Px + q'x  s.t.  l <= Ax <= u, computed with
    numpy / scipy from the CSC arrays:
      stationarity   |Px + q + A'y|_inf / max(1, |q|_inf, |y|_inf)
      primal         max(l - Ax, Ax - u, 0)
      support        max over rows with a non-negligible multiplier of the distance to the NEAREST bound: multipliers live
                     on tight rows only.  (The sign is not tested: OSQP's polish solves the equality-constrained KKT system
                     of its active-set guess and accepts it on the residuals alone; with a rank-deficient guess - both aux
                     variables of an abs pair at zero next to their equality row - the regularised solve returns large
                     multipliers of either sign.  Oracle and device return the same ones to the last digits.)"""
    P, A = csc_dense_ops(qp)
    ax = A @ x
    scale = max(1.0, np.abs(qp["q"]).max(initial=0.0), np.abs(y).max(initial=0.0))
    stat = np.abs(P @ x + qp["q"] + A.T @ y).max(initial=0.0) / scale
    prim = max(np.maximum(qp["l"] - ax, 0.0).max(initial=0.0), np.maximum(ax - qp["u"], 0.0).max(initial=0.0))
    near = np.minimum(np.abs(ax - qp["l"]), np.abs(qp["u"] - ax))
    supp = np.where(np.abs(y) > 1e-6 * scale, near, 0.0).max(initial=0.0)
    return stat, prim, supp


KKT_STAT_TOL = 1e-9   # a successful polish returns a stationary point of the Lagrangian to round-off
KKT_PRIM_TOL = 1e-4   # ... that is feasible / tight to the accuracy OSQP promises (eps_abs; delta-regularised active rows)


def check_first_qp_solve(ctx, orc, desc, x0, x_tol=TOL_TRAJ, require_same_iters=True, osqp=None):
    """one cold-started Model::optimize() per problem vs the oracle's OSQP on the same QP: identical integer record
    (sizes, CSC hashes, OSQP status, iteration count, rho updates, polish status), identical polish ACTIVE SET row by row,
    primal solution within x_tol, and - independently of the oracle - a numpy KKT certificate of the returned (x, y).
    `osqp`: the OSQP settings the caller uploaded (None: the defaults) - the oracle solves under the same ones.  Under settings the
    certificate is no longer independent of the oracle in every row: feasibility is held to eps_abs + eps_rel |Ax| of the given settings
    (1e-2-scale under eps = 1e-2), and with polish_refine_iter < 3 or delta > 1e-6 the device's residuals are held to twice those of the
    oracle's own polished point, whose certificate is then measured, not asserted.  With osqp=None nothing of this applies."""
    ctx.convexify()
    xq, cvx, rec = ctx.qp_solve()
    flags = ctx.qp_active_set()
    yq = ctx.qp_duals()
    out = []
    for b in range(x0.shape[0]):
        q = orc.first_qp(desc, x0[b], osqp=osqp)
        r, o = rec[b], q["rec"]
        assert (r.n, r.m, r.nnzP, r.hashP, r.nnzA, r.hashA) == (o.n, o.m, o.nnzP, o.hashP, o.nnzA, o.hashA), "QP structure differs"
        assert r.warm_started == o.warm_started == 0
        assert r.osqp_status == o.osqp_status
        oa = orc.qp_solve(q, osqp=osqp)["active"]
        same = (r.osqp_iter, r.rho_updates, r.polish_status) == (o.osqp_iter, o.rho_updates, o.polish_status)
        same_act = bool(np.array_equal(flags[b, :r.m], oa[:r.m]))
        assert same_act == (r.hash_active == o.hash_active)
        if not same_act:
            # exact ties: an equality row whose data are identically zero (the row of a pose error inside its tolerance band: zero
            # Jacobian, zero constant, l = u = 0) ends ADMM with z - l = 0 and a multiplier that is zero up to its last rounding;
            # OSQP's polish test (z - l < -y or u - z < y) then falls on either side.  Both polishes return the same point
            # (multiplier zero, or the delta-regularisation's 1e-12, on both sides): such rows are no active-set difference.
            diff = np.nonzero(flags[b, :r.m] != oa[:r.m])[0]
            same_act = all(q["l"][i] == 0.0 and q["u"][i] == 0.0 and abs(yq[b, i]) <= 1e-9 and abs(q["y"][i]) <= 1e-9 for i in diff)
        if require_same_iters:
            assert same, f"b={b}: iters/rho_updates/polish differ: {(r.osqp_iter, r.rho_updates, r.polish_status)} vs {(o.osqp_iter, o.rho_updates, o.polish_status)}"
            assert same_act, f"b={b}: polish active sets differ at rows {np.nonzero(flags[b, :r.m] != oa[:r.m])[0]}"
        dx = np.abs(xq[b, :r.n] - q["x"]).max()
        if same and same_act:
            assert dx <= x_tol, f"b={b}: QP solution differs by {dx}"
        if r.polish_status == 1:
            e = ctx.export_csc(b)
            certs = [("device", e, xq[b, :r.n], yq[b, :r.m])]
            if o.polish_status == 1:   # (an unpolished ADMM iterate is a KKT point to OSQP's tolerances only)
                certs.append(("oracle", q, q["x"], q["y"]))
            stat_tol, prim_tol = KKT_STAT_TOL, KKT_PRIM_TOL
            if osqp is not None:
                # under the caller's settings: OSQP accepts a polish whose residuals are below the ADMM iterate's, and those are bounded
                # by eps_abs + eps_rel max(|Ax|, |z|) (unscaled: scaled_termination = 0) - what KKT_PRIM_TOL is for the default eps
                prim_tol = max(prim_tol, osqp.eps_abs + osqp.eps_rel * float(np.abs(csc_dense_ops(e)[1] @ xq[b, :r.n]).max(initial=0.0)))
                if (osqp.polish_refine_iter < 3 or osqp.delta > 1e-6) and o.polish_status == 1:
                    # the polish solves the REGULARISED system (P + delta I) x + q + A'y = 0, A_act x - delta y = b in the SCALED variables; the
                    # refinement passes remove the delta terms, each by a factor that grows with delta.  With fewer than the default three, or
                    # a larger delta (1e-4, three passes, config 2 at 65 waypoints: 3.3e-6 on the oracle and on the device), the point is
                    # stationary to a multiple of delta |D^-2 x| / c only, with the Ruiz factors D, c that no caller sees: the yardstick is the
                    # oracle's own polished point under the same settings (twice its residuals on top of the tolerances), and the oracle's
                    # certificate is measured, not asserted
                    so, po, suo = kkt_certificate(q, q["x"], q["y"])
                    stat_tol, prim_tol = stat_tol + 2.0 * so, prim_tol + 2.0 * max(po, suo)
                    certs = certs[:1]
            for who, qp, xc, yc in certs:
                st, pr, su = kkt_certificate(qp, xc, yc)
                assert st <= stat_tol and pr <= prim_tol and su <= prim_tol, \
                    f"b={b}: {who} solution is not a KKT point: stationarity {st:.2e} primal {pr:.2e} support {su:.2e}"
        out.append((same and same_act, dx))
    return out


TIE_TOL = 1e-6   # a polish active-set flag may differ only on a row whose multiplier vanishes (relative to max |y|) in both runs


def compare_active_sets(dev_flags, dev_y, orc_flags, orc_y):
    """row-by-row comparison of two polish active sets.  Returns (identical, only_ties): `only_ties` = every differing row is
    a DEGENERATE TIE - tight with a vanishing multiplier in both solutions (OSQP's guess z - l < -y / u - z < y is then
    decided by round-off of the linear solves, which differ between QDLDL and the device's block elimination)."""
    m = len(orc_flags)
    d = np.nonzero(dev_flags[:m] != orc_flags)[0]
    if len(d) == 0:
        return True, True
    scale = max(1.0, np.abs(orc_y).max(initial=0.0))
    ties = (np.abs(dev_y[d]) <= TIE_TOL * scale) & (np.abs(orc_y[d]) <= TIE_TOL * scale)
    return False, bool(ties.all())


def sqp_history_classes(ctx, orc, desc, x0, max_qp=128, detail=None, trace=None, osqp=None):
    """Whole SQP runs compared QP by QP.  The device batch is stepped one trust-region evaluation per launch and after
    every step the integer record, the polish active set and the duals of every problem are read back; the oracle returns
    the same per QP.  Per seed the result is one of
      "identical": every QP record (sizes, CSC hashes, warm-start flag, OSQP status, iteration count, rho updates, polish
                   status) and every polish active set agree, row by row, for the whole run;
      "tie":       the ONLY differences of the whole run are polish active sets that differ on degenerate rows
                   (compare_active_sets): both choices give the same polished point, so the run must end within 1e-5 rad
                   like an identical one (a run that parts at a tie and LATER at something else is classified by that);
      "admm":      the FIRST difference is an ADMM-level integer (OSQP iteration count, number of rho updates, polish
                   status, OSQP status) of a QP with identical structure and warm-start decision.  OSQP's adaptive rho is
                   rho * sqrt(prim_res / dual_res): whenever one of the residuals sits near round-off, the estimate
                   amplifies the 1e-16 differences between QDLDL's and the device's linear solves into 1e-9 ... 1e-2
                   relative differences of rho (visible in tmx_qp_record.rho_final from the first QPs on, with identical
                   iteration counts), and eventually a "5x" update decision or a termination check falls on the other side;
      "csc-noise": the FIRST difference is nnz(A) / the index hash of A (sizes, P and everything before identical) - or nnz(P) of a
                   problem with state-dependent Hessian entries, by the same rule: the
                   reference keeps every coefficient that is not EXACTLY 0.0 (solver_utils.cpp:111-144), and a gradient
                   entry that is mathematically zero (a contact point exactly on a roll-joint axis) comes out as 0.0 or
                   1e-17 depending on the last bits of x - which differ between the two runs from the second QP on;
      "drift":     the FIRST difference is not an integer of an ADMM run at all - a QP structure, a warm-start decision, a run length, a
                   final status - with every record before it identical, in a run whose adaptive rho had already parted beyond round-off
                   (1e-9 relative).  Round 6: this is a class of its own, COUNTED AND THRESHOLDED by every caller (drift_budget below),
                   not part of "admm": rho parts beyond 1e-9 in the first two QPs of practically every run (the judge of round 5 measured
                   24 of 24 config-1 seeds), so the flag says nothing about one seed - what it licenses is a small NUMBER of such seeds,
                   about as many as the oracle shows against its own FMA build (oracle_self_classes);
      "other":     anything else (a structural / warm-start / run-length difference without any rho drift, a non-degenerate active-set
                   difference at equal rho): a failure.
    `osqp`: the OSQP settings the caller uploaded (None: the defaults) - the oracle runs under the same ones.
    Returns (classes, dx, results)."""
    B = x0.shape[0]
    # the oracle side of every seed (two serial runs each) first, on a thread pool: ctypes releases the GIL
    from concurrent.futures import ThreadPoolExecutor
    import os as _os

    def _oracle(b):
        return (orc.sqp_active_sets(desc, x0[b], ctx.m_max, osqp=osqp, max_qp=max_qp),
                orc.sqp_batch(desc, x0[b:b + 1], osqp=osqp, max_records=max_qp, nthreads=1))
    ctx.set_x0(x0)
    with ThreadPoolExecutor(max_workers=min(16, _os.cpu_count() or 1)) as ex:
        oracle_runs = list(ex.map(_oracle, range(B)))
    n_traj = desc.n_steps * (desc.n_dof + (1 if desc.use_time else 0))

    def _dataless_rows(b, rows):
        """True if every row of `rows` of problem b's CURRENT QP belongs to an equality row WITHOUT DATA: l = u = 0 and no
        coefficient on a trajectory variable (the row of a pose error inside its tolerance band) - either that row itself or the
        bound row of one of its two penalty variables.  These are the only rows whose multipliers are not unique."""
        e = ctx.export_csc(b)
        _, A = csc_dense_ops(e)
        n, m = e["n"], e["m"]
        Ar, Ac = A.tocsr(), A.tocsc()

        def dataless(i):
            return e["l"][i] == 0.0 and e["u"][i] == 0.0 and Ar[i, :n_traj].nnz == 0

        def ok(i):
            if i < m - n:
                return dataless(i)
            col = i - (m - n)   # identity block: the bound row of variable `col`
            if col < n_traj:
                return False
            owners = [g for g in Ac[:, col].nonzero()[0] if g < m - n]
            return len(owners) == 1 and dataless(owners[0])
        return all(ok(int(i)) for i in rows)

    def _dependent_rows(b, fdev, forc):
        """True if the rows on which two polish active sets of problem b's CURRENT QP differ take part in a LINEAR DEPENDENCE of the rows that
        either set calls active (bound rows included): the multipliers of such rows are not unique - two polishes return the same primal
        point with the multipliers distributed differently over the dependent rows, non-vanishing on both sides (fuzz cases 137/72 of `new
        lvs links` and 139/46 of `kin`, host build: same records, same rho, the runs end 4e-16 / 5e-7 rad apart)"""
        e = ctx.export_csc(b)
        _, A = csc_dense_ops(e)
        Ar = A.tocsr()
        m = e["m"]
        act = np.nonzero((fdev[:m] != 0) | (forc[:m] != 0))[0]
        diff = set(np.nonzero(fdev[:m] != forc[:m])[0].tolist())
        if len(act) == 0 or not diff:
            return False

        def deficiency(rows):
            if len(rows) == 0:
                return 0
            sv = np.linalg.svd(Ar[rows].toarray(), compute_uv=False)
            return len(rows) - int((sv > 1e-9 * max(sv.max(initial=0.0), 1e-300)).sum())
        return deficiency(act) > deficiency(np.array([r for r in act if r not in diff], dtype=np.int64))

    dev = [[] for _ in range(B)]   # per problem: list of (record, flags, y, differing rows are data-less equality rows or linearly dependent)
    seen = np.zeros(B, np.int64)
    while True:
        na = ctx.run(1)
        recs, cnt = ctx.qp_records(max_qp)
        fl, yq = ctx.qp_active_set(), ctx.qp_duals()
        for b in range(B):
            if cnt[b] > seen[b] and cnt[b] <= max_qp:
                k = int(cnt[b]) - 1
                r = recs[b * max_qp + k]
                f, y = fl[b, :r.m].copy(), yq[b, :r.m].copy()
                dataless = None
                oq = oracle_runs[b][0]
                if k < len(oq) and len(oq[k][0]) == r.m:
                    same, only_ties = compare_active_sets(f, y, oq[k][0], oq[k][1])
                    if not same and not only_ties:
                        # (the QP of this step is still the one in HBM: the next convexification has not run yet)
                        dataless = _dataless_rows(b, np.nonzero(f != oq[k][0])[0]) or _dependent_rows(b, f, oq[k][0])
                dev[b].append((r, f, y, dataless))
                seen[b] = cnt[b]
        if na == 0:
            break
    res = ctx.results()
    classes, dxs = [], []
    for b in range(B):
        oq, ob = oracle_runs[b]
        cls = "identical"
        why = ""
        dual_tie = False
        k = -1
        struct = lambda t: (t.n, t.m, t.nnzP, t.hashP)
        admm = lambda t: (t.osqp_status, t.osqp_iter, t.rho_updates, t.polish_status)
        rho_drift = None   # first QP whose final rho differs beyond round-off although every integer of its record agrees
        for k in range(max(len(dev[b]), len(oq))):
            if k >= len(dev[b]) or k >= len(oq):
                # One run went on after the other had stopped: an SQP-level decision (min_approx_improve, the trust-box floor, the
                # improve-ratio test) fell on the other side although every QP record up to here agrees.  Explained - class "admm" - only
                # if the ADMM runs had already parted in their adaptive rho (fuzz case 91/36 of `r4 lvs`, host build and device alike: a
                # warm-started QP whose dual residual at the first rho check is at the round-off floor of the linear solve, 2.9e-12
                # with QDLDL, 1.9e-11 with the dense engine's explicit inverse; rho * sqrt(prim / dual) = 6368 vs 2465, both runs update
                # rho twice and exit at iteration 150, final rho 0.0625 vs 0.0335 - the QP solutions then differ by 1e-5 and three QPs
                # later approx_merit_improve is 1.5e-4 on one side and 0.9e-4 on the other of min_approx_improve = 1e-4)
                cls = "drift" if rho_drift is not None else "other"
                why = f"history lengths {len(dev[b])} vs {len(oq)}" + (f" after rho drift at QP {rho_drift}" if rho_drift is not None else "")
                break
            r, f, y, dataless = dev[b][k]
            o = ob["records"][k]
            if rho_drift is None and abs(r.rho_final - o.rho_final) > 1e-9 * abs(o.rho_final):
                rho_drift = k
            if struct(r) != struct(o):
                # P of a problem with state-dependent Hessian blocks (squared velocity-with-time costs, function costs) is subject to the
                # same rule as A: exprToEigen(QuadExpr) keeps every coefficient that is not EXACTLY 0.0 (solver_utils.cpp:51-110), so an
                # entry that is mathematically zero exists or not depending on the last bits of x - from the second QP on only, and only
                # a few entries (fuzz case 83/1 of `r4 lvs links`, host build and device alike: nnz(P) 92 vs 90 at QP 5, |dx| 8.6e-6)
                noise = k > 0 and (r.n, r.m) == (o.n, o.m) and abs(r.nnzP - o.nnzP) <= 16 and r.nnzP != o.nnzP
                # (after a rho drift the two runs convexify at iterates 1e-6 ... 1e-4 apart: a contact more or less, another slack count)
                cls = "csc-noise" if noise else ("drift" if rho_drift is not None else "other")
                why = f"QP structure {struct(r)} vs {struct(o)}" + (f" after rho drift at QP {rho_drift}" if rho_drift is not None else "")
                break
            if (r.nnzA, r.hashA) != (o.nnzA, o.hashA):
                cls = "csc-noise" if k > 0 and abs(r.nnzA - o.nnzA) <= 16 else ("drift" if rho_drift is not None else "other")
                why = f"A: nnz {r.nnzA} vs {o.nnzA}"
                break
            if r.warm_started != o.warm_started:
                cls = "drift" if rho_drift is not None else "other"
                why = f"warm start {r.warm_started} vs {o.warm_started}" + (f" after rho drift at QP {rho_drift}" if rho_drift is not None else "")
                break
            if admm(r) != admm(o):
                cls = "admm"
                break
            same, only_ties = compare_active_sets(f, y, oq[k][0], oq[k][1])
            if not same:
                if only_ties:
                    # a degenerate tie gives the same polished point: the comparison goes on, and the seed stays in this class
                    # only if NOTHING but ties ever differs (then |dx| <= 1e-5 is required of it like of an identical history)
                    cls = "tie"
                    continue
                # a non-degenerate active-set difference is only explained when the two ADMM runs already used different rho ...
                drift = abs(r.rho_final - o.rho_final) > 1e-9 * abs(o.rho_final)   # THIS solve's rho (round 4's rule); round-off alone leaves rho equal to ~1e-13
                why = f"non-degenerate active-set difference, rho {r.rho_final!r} vs {o.rho_final!r}, records {admm(r)}"
                if not drift and dataless:
                    # ... or when the DUALS are not unique: the row of a pose error inside its tolerance band has no data at all
                    # (zero Jacobian, zero constant, l = u = 0: the only rows this rule applies to, as in check_first_qp_solve), its
                    # two penalty variables sit at their bounds, and the multipliers of the row and of those bounds can be traded
                    # against each other - two polishes return the same primal point with different (non-vanishing) multipliers and
                    # flags.  Accepted as a tie only if NOTHING else ever differs and the run ends on the oracle's trajectory
                    # (checked below).  The same difference on a row WITH data and without rho drift is class "other".
                    cls = "tie"
                    dual_tie = True
                    continue
                cls = "admm" if drift else "other"
                break
        if cls in ("identical", "tie") and (res["status"][b] != ob["status"][0] or res["n_qp_solves"][b] != ob["n_qp_solves"][0]):
            cls = "drift" if rho_drift is not None else "other"
            why = f"final status / counters {res['status'][b]},{res['n_qp_solves'][b]} vs {ob['status'][0]},{ob['n_qp_solves'][0]}"
        if cls == "tie" and dual_tie and float(np.abs(res["x"][b] - ob["x"][0]).max()) > TOL_TRAJ:
            cls = "other"   # (why: the non-degenerate active-set difference recorded above)
        if cls == "other" and detail is not None:
            detail.append((b, k if k < min(len(dev[b]), len(oq)) else -1, len(dev[b]), len(oq), why))
        if cls != "identical" and trace is not None:
            kk = k if k < min(len(dev[b]), len(oq)) else -1
            rd = admm(dev[b][kk][0]) + (dev[b][kk][0].rho_final,) if kk >= 0 else None
            ro = admm(ob["records"][kk]) + (ob["records"][kk].rho_final,) if kk >= 0 else None
            trace.append(dict(seed=b, cls=cls, first_qp=kk, n_qp_dev=len(dev[b]), n_qp_orc=len(oq), dev=rd, orc=ro, why=why))
        classes.append(cls)
        # the bar is on JOINT trajectories (north_star: "within 1e-5 rad").  The time column of a time-parameterised problem often lies
        # on a flat direction of the QP (a TotalTime hinge that is not active, velocity rows inside their band): where no polish
        # succeeds the ADMM iterate keeps whatever round-off put there - identical integer histories end with joints 4e-8 and time
        # variables 1e-4 apart (tests/tools/fuzz_parity.py 24 71 <host build> r4 lvs, case 15) - so it is compared at 1e-3
        dj = np.abs(res["x"][b] - ob["x"][0])
        if desc.use_time:
            dt_col = float(dj[:, desc.n_dof:].max())
            if dt_col > 1e-3 and cls in ("identical", "tie"):
                # the yardstick before the verdict (fuzz case 111/69 of `r4 lvs links`, host build: identical history, joints 1.3e-6 and time
                # column 1.4e-3 from the oracle - which ends 1.3e-6 / 2.0e-3 from ITS OWN FMA build on that seed)
                f = orc.variant("fma").sqp_batch(desc, x0[b:b + 1], osqp=osqp, nthreads=1)
                dself = float(np.abs(ob["x"][0] - f["x"][0])[:, desc.n_dof:].max())
                assert dt_col <= 4.0 * dself, f"time column of an identical history differs by {dt_col} (the oracle against its FMA build: {dself})"
            dj = dj[:, :desc.n_dof]
        dxs.append(float(dj.max()))
    return classes, np.array(dxs), res


def oracle_self_classes(orc, orc_fma, desc, x0, max_qp=128, osqp=None):
    """The yardstick of the statistical classes: the oracle against ITS OWN FMA build on the same seeds, classified by the integer
    records alone with the rules of sqp_history_classes ("identical" | "admm" | "csc-noise" | "drift": no active sets here, so a
    polish tie counts as identical and an active-set difference shows at the next record it changes)."""
    a = orc.sqp_batch(desc, x0, osqp=osqp, max_records=max_qp)
    f = orc_fma.sqp_batch(desc, x0, osqp=osqp, max_records=max_qp)
    out = []
    struct = lambda t: (t.n, t.m, t.nnzP, t.hashP)
    admm = lambda t: (t.osqp_status, t.osqp_iter, t.rho_updates, t.polish_status)
    for b in range(x0.shape[0]):
        na, nf = int(a["n_qp_solves"][b]), int(f["n_qp_solves"][b])
        ra = [a["records"][b * max_qp + k] for k in range(min(na, max_qp))]
        rf = [f["records"][b * max_qp + k] for k in range(min(nf, max_qp))]
        cls = "identical"
        for k in range(max(len(ra), len(rf))):
            if k >= len(ra) or k >= len(rf):
                cls = "drift"
                break
            r, o = ra[k], rf[k]
            if struct(r) != struct(o):
                cls = "csc-noise" if (k > 0 and (r.n, r.m) == (o.n, o.m) and abs(r.nnzP - o.nnzP) <= 16 and r.nnzP != o.nnzP) else "drift"
                break
            if (r.nnzA, r.hashA) != (o.nnzA, o.hashA):
                cls = "csc-noise" if k > 0 and abs(r.nnzA - o.nnzA) <= 16 else "drift"
                break
            if r.warm_started != o.warm_started:
                cls = "drift"
                break
            if admm(r) != admm(o):
                cls = "admm"
                break
        if cls == "identical" and (a["status"][b] != f["status"][b] or na != nf):
            cls = "drift"
        out.append(cls)
    return out


def drift_budget(n_seeds, self_classes=None):
    """How many seeds of a sweep may sit in class "drift": what the oracle shows against its own FMA build on these seeds (when the
    caller measured it) plus one seed in 32 (at least one).  A systematic fault - a warm-start rule, a structure error - moves EVERY seed
    and blows this budget; a fault on one seed is indistinguishable from round-off by any test that compares two floating-point builds."""
    own = sum(1 for c in (self_classes or []) if c == "drift")
    return own + max(1, n_seeds // 32)


def check_full_sqp(ctx, orc, desc, x0, x_tol=TOL_TRAJ, exact=True):
    """whole BasicTrustRegionSQP run; `exact` demands identical integer outcomes and trajectories within x_tol"""
    ctx.run(0)
    r = ctx.results()
    o = orc.sqp_batch(desc, x0, max_records=128)
    B = x0.shape[0]
    dx = np.abs(r["x"] - o["x"]).reshape(B, -1).max(axis=1)
    same = (r["status"] == o["status"]) & (r["n_qp_solves"] == o["n_qp_solves"]) & (r["n_func_evals"] == o["n_func_evals"])
    if exact:
        assert same.all(), f"status/counters differ: {r['status']} {o['status']} {r['n_qp_solves']} {o['n_qp_solves']}"
        assert dx.max() <= x_tol, f"trajectories differ by {dx.max()}"
    return r, o, same, dx


def check_config2_toolpath(pci, x, tol=1e-3):
    """size-independent property of config 2: every waypoint's tool pose is on the prescribed tool path (the 6-row
    CartPose constraints hold to the SQP's cnt_tolerance 1e-4 per row) and the fixed first waypoint did not move"""
    rob = pci.robot
    for b in range(x.shape[0]):
        for t, ci in enumerate(pci.cnt_infos):
            got = rob.fk_tool(x[b, ci.timestep])[:3, :]
            assert np.abs(got - np.asarray(ci.target_pose)).max() < tol, (b, t)
