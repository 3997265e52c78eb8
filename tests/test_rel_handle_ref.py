"""The pins that make the GPU comparison of test_gpu_relative.py meaningful, computed with
rel_ref.lm_with_relatives alone (CPU oracle, no GPU): on every parity scene the reference
loop both accepts and rejects steps, no gain ratio lies near a threshold of the controller
(a last-bit difference cannot flip a decision), and the factors move the first trial cost
far beyond the comparison's tolerance."""
import numpy as np
import pytest

import rel_handle_cases as cases

PARITY = ["group150", "chunk60", "small30", "blind30"]


@pytest.mark.parametrize("name", PARITY)
def test_reference_accepts_and_rejects_far_from_the_thresholds(built, name):
    rows = cases.reference(name)[0]
    assert len(rows) == cases.ITERS
    status = [r.iteration_status for r in rows]
    print(name, status, ["%.3g" % r.rho for r in rows])
    assert 2 in status and (0 in status or 1 in status), status
    for r in rows:
        for thr in (0.25, 0.5):
            assert abs(r.rho - thr) > 0.5 * thr, (name, r.rho)


@pytest.mark.parametrize("name", PARITY)
def test_factors_move_the_first_trial_cost(built, name):
    a = cases.reference(name)[0][0].trial_cost
    b = cases.plain_oracle_rows(name)[0].trial_cost
    print(name, a, b)
    assert abs(a - b) > 1e-4 * abs(b)


def test_factor_set_has_every_kind_of_pair(built):
    pr, rels = cases.case("small30")
    fixed = np.asarray(pr["pose_fixed"]) != 0
    j, k = rels["j"], rels["k"]
    assert (fixed[j] & ~fixed[k]).any() and (~fixed[j] & fixed[k]).any() and not (fixed[j] & fixed[k]).any()
    pairs = list(zip(j.tolist(), k.tolist()))
    assert any((b, a) in pairs for a, b in pairs)                       # one pair in both orientations
    assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs)
    assert max(abs(a - b) for a, b in pairs) > 10                      # far pairs
    # the blind pose is held by its two chain factors only
    blind = cases.case("blind30")[0]
    assert not (np.asarray(blind["obs_pose"]) == cases.BLIND).any()
    assert sorted(p for p in pairs if cases.BLIND in p) == [(cases.BLIND, cases.BLIND - 1),
                                                             (cases.BLIND + 1, cases.BLIND)]
