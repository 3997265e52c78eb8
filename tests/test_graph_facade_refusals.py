"""What the graph methods of the Python facades refuse BEFORE a graph is created, for the SE(3)
and the Sim(3) graph and both solver classes: the exception type and the whole message.  No GPU is
touched: every refusal here is raised on the host from the registered poses and factors alone.
"""
import re

import numpy as np
import pytest

from bundle_adjustment_solver_amd.solver import (FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor,
                                                 Options)

CLASSES = [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor]
# kind -> the method names, the word in the messages, the information's width, the second
# sigma_pixel of the mixed case
KINDS = {
    "se3": dict(add="AddRelativePose", solve="SolvePoseGraph", cov="ComputePoseGraphCovariance",
                gate="GateLoopClosures", weights="GetRelativeWeights", width=6, other=2.0),
    "sim3": dict(add="AddRelativeSim3", solve="SolveSim3Graph", cov="ComputeSim3GraphCovariance",
                 gate="GateSim3LoopClosures", weights="GetRelativeSim3Weights", width=7, other=0.5),
}
NO_POINTER = "There is no pointer in the BA pose pool."


def solver(cls):
    """three 4x4 identity poses, registered as objects -> (solver, the pose objects)"""
    s = cls()
    poses = [np.eye(4) for _ in range(3)]
    for p in poses:
        s.AddPose(p)
    return s, poses


def factor(kd, j, k, **more):
    return dict(pose_j=j, pose_k=k, measurement=np.eye(4), information=np.eye(kd["width"]), **more)


def add(s, kd, j, k, sigma_pixel):
    getattr(s, kd["add"])(j, k, np.eye(4), np.eye(kd["width"]), sigma_pixel=sigma_pixel)


def raises(exc, message):
    """the exact type (no subclass) and the whole message"""
    ctx = pytest.raises(exc, match="^" + re.escape(message) + "$")
    return ctx


def calls(s, kd, poses):
    return [(kd["solve"], lambda: getattr(s, kd["solve"])(Options())),
            (kd["cov"], lambda: getattr(s, kd["cov"])([poses[1]], [(poses[1], poses[2])])),
            (kd["gate"], lambda: getattr(s, kd["gate"])([factor(kd, poses[1], poses[2])]))]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_nothing_added(cls, kind):
    kd = KINDS[kind]
    want = "%s: poses (AddPose) and factors (" + kd["add"] + ") must be added first"
    # neither poses nor factors, then poses without factors
    for s, poses in ((cls(), [0, 1, 2]), solver(cls)):
        registered = s.num_total_poses_ > 0
        for name, call in calls(s, kd, poses):
            if not registered and name != kd["solve"]:
                continue   # an unregistered pose in the selection is refused first (test_unknown_pose)
            with raises(RuntimeError, want % name) as e:
                call()
            assert type(e.value) is RuntimeError


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_weights_before_a_solve(cls, kind):
    kd = KINDS[kind]
    s, poses = solver(cls)
    add(s, kd, poses[1], poses[0], 1.0)
    with raises(RuntimeError, "%s: %s has not run" % (kd["weights"], kd["solve"])) as e:
        getattr(s, kd["weights"])()
    assert type(e.value) is RuntimeError


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_mixed_sigma_pixel_among_the_factors(cls, kind):
    kd = KINDS[kind]
    s, poses = solver(cls)
    add(s, kd, poses[1], poses[0], 1.0)
    add(s, kd, poses[2], poses[1], kd["other"])
    want = ("%s: the factors and candidates were given with sigma_pixel = 1 and %g; a covariance in the caller's "
            "units needs one value" % (kd["cov"], kd["other"]))
    assert want.count("sigma_pixel = 1 and 2;") + want.count("sigma_pixel = 1 and 0.5;") == 1   # the %g form
    with raises(RuntimeError, want) as e:
        getattr(s, kd["cov"])([poses[1]])
    assert type(e.value) is RuntimeError


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_candidate_with_another_sigma_pixel(cls, kind):
    kd = KINDS[kind]
    s, poses = solver(cls)
    add(s, kd, poses[1], poses[0], 1.0)
    want = ("%s: the factors and candidates were given with sigma_pixel = 1 and 3; a covariance in the caller's "
            "units needs one value" % kd["gate"])
    with raises(RuntimeError, want) as e:
        getattr(s, kd["gate"])([factor(kd, poses[2], poses[1], sigma_pixel=3.0)])
    assert type(e.value) is RuntimeError


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_unknown_pose(cls, kind):
    kd = KINDS[kind]
    s, poses = solver(cls)
    add(s, kd, poses[1], poses[0], 1.0)
    stranger = np.eye(4)
    for call in (lambda: getattr(s, kd["cov"])([poses[1], stranger]),
                 lambda: getattr(s, kd["cov"])([poses[1]], [(poses[1], stranger)]),
                 lambda: getattr(s, kd["cov"])([], [(stranger, poses[2])]),
                 lambda: getattr(s, kd["cov"])([7]),
                 lambda: getattr(s, kd["gate"])([factor(kd, poses[1], stranger)]),
                 lambda: getattr(s, kd["gate"])([factor(kd, stranger, poses[2])])):
        with raises(RuntimeError, NO_POINTER) as e:
            call()
        assert type(e.value) is RuntimeError


@pytest.mark.parametrize("cls", CLASSES)
def test_wrong_anchor_count(cls):
    s, poses = solver(cls)
    # without factors "must be added first" comes before the anchors are looked at
    with raises(RuntimeError, "SolveSim3Graph: poses (AddPose) and factors (AddRelativeSim3) must be added first") as e:
        s.SolveSim3Graph(Options(), point_anchors=[0])
    assert type(e.value) is RuntimeError
    add(s, KINDS["sim3"], poses[1], poses[0], 1.0)
    assert s.num_total_points_ == 0
    with raises(ValueError, "SolveSim3Graph: one anchor (or None) per registered point") as e:
        s.SolveSim3Graph(Options(), point_anchors=[0])
    assert type(e.value) is ValueError
