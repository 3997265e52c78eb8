"""CPU test of the float64 one-step references (pose_only6_ref.py,
planar_pose_ref.py at float64) and of the tolerance table of
onestep_cases.py, for every case test_gpu_pose_only_onestep.py runs: the
project's independent fp32 restatement of the same loop (the C++ oracle for
6-DoF, planar_pose_ref at float32 for planar) lies within MEASURED = TOL / K of
the float64 reference in every compared quantity, the masks are identical, and
the scene's preconditions hold (every edge >= 0.05 px from both thresholds;
where the cost is compared, every probe's share of it >= 8x the cost
tolerance).  No GPU."""
import numpy as np
import pytest

import onestep_cases as oc


def check(sc, max_iter, compare_cost=True):
    ref = oc.ref64(sc, max_iter)
    f32 = oc.ref32(sc, max_iter)
    cls = oc.size_class(sc["n"])
    oc.check_preconditions(sc, ref, oc.tol(sc)["cost"] if compare_cost else None)
    assert ref["success"] and f32["success"]
    assert ref["n_iter"] == f32["n_iter"] == max_iter and not ref["converged"]
    dev = oc.deviations(f32, ref)
    for q, v in dev.items():
        bound = oc.MEASURED[cls][q]
        if q == "cost":
            if not compare_cost:
                continue
            if bound is None:     # large class: the kernel's own a-priori bound
                if oc.sequential_yardstick(sc):
                    assert v < 1e-2     # the sequential sum: off by ~1e-3, no yardstick
                    continue
                bound = oc.COST_LARGE
        assert v <= bound, (q, v, bound)
    want = oc.expected_classes(sc)
    for k in oc.mask_keys(sc):
        assert np.array_equal(ref[k], f32[k]), k
        assert np.array_equal(ref[k], want[k]), k
    return dev


@pytest.mark.parametrize("opt", ["A", "B"])
@pytest.mark.parametrize("variant", oc.VARIANTS)
def test_one_iteration_cases(built, variant, opt):
    for n in oc.sizes(variant):
        check(oc.scene(variant, n, opt), 1, oc.cost_compared(opt, n))


@pytest.mark.parametrize("variant", oc.VARIANTS)
def test_three_iteration_cases(built, variant):
    for n in oc.SIZES_3ITER:
        check(oc.scene(variant, n, "B"), 3)


@pytest.mark.parametrize("opt", ["A", "B"])
@pytest.mark.parametrize("variant", oc.VARIANTS)
def test_batch_cases(built, variant, opt):
    for sc in oc.batch(variant, opt):
        if sc is not None:
            check(sc, 1, oc.cost_compared(opt, sc["n"]))


def test_probe_indices_cover_the_work_split():
    assert list(oc.probe_indices(3)) == [0, 1, 2]
    assert list(oc.probe_indices(2)) == [0, 1]
    p = oc.probe_indices(262145)
    for i in (0, 63, 64, 1023, 1024, 2047, 2048, 65535, 65536, 66559, 131072, 132095, 196608,
              197631, 262144, 262143):
        assert i in p
    assert p.max() == 262144 and len(set(p)) == len(p)
    sc = oc.scene("stereo6", 2049, "A")
    assert 1024 in sc["no_right"] and 2048 in sc["no_right"]
    assert len(sc["no_right"]) * 2 in range(len(sc["probes"]) - 2, len(sc["probes"]) + 4)
    assert sc["uv_right"][sc["zero_idx"], 0] == 0.0
    assert (sc["uv_right"][sc["no_right"]] < 0).any(axis=1).all()
    assert not (sc["uv_right"][sc["no_right"]] < 0).all(axis=1).any()


def test_float32_planar_restatement_is_unchanged():
    """planar_pose_ref at its default dtype still computes in float32."""
    sc = oc.scene("stereo3", 65, "A")
    out = oc.ref32(sc, 2)
    assert out["T12"].dtype == np.float32 and out["debug"].dtype == np.float32
    assert oc.ref64(sc, 2)["T12"].dtype == np.float64
