"""Every form of VectorAgentManager's ONE collect loop against every other, byte for byte (the matrix: tests/vector_collect_forms.py).

Forms: DiscreteFF with and without `fused_step` on the host and on the device interface (four); the diagonal-Gaussian head and
MultiDiscreteFF with bins (2, 7, 3) on both interfaces (two each).  n_agents 1, 3 and 16; three consecutive collects on the same
manager (T = 1, 9 and a ragged 5): the flush step that is also the first step, two crossings of the statistics cadence, and the state
carried from one collect to the next.  Features one at a time, and masks with critic observations together."""
import pytest

import vector_collect_forms as F

pytestmark = pytest.mark.gpu


def _hold_together(results):
    """{form name: [(outputs, bootstrap)] per collect}: every form to the first one, output by output."""
    names = sorted(results)
    ref = results[names[0]]
    for name in names[1:]:
        for i, ((want, _), (got, _)) in enumerate(zip(ref, results[name])):
            assert want.keys() == got.keys()
            for key in want:
                assert want[key] == got[key], f"collect {i}: {key} of {name} differs from {names[0]}"
    for i in range(len(ref)):   # bootstrap: the host forms' sparse answer among themselves, the device forms' dense rows at those steps
        boots = [results[n][i][1] for n in names]
        if all(b is None for b in boots):
            continue
        sparse = [b for b in boots if "steps" in b]
        for b in boots:
            if "steps" in b:
                assert b["steps"].tobytes() == sparse[0]["steps"].tobytes() and b["rows"].tobytes() == sparse[0]["rows"].tobytes(), f"collect {i}"
            else:
                F.check_bootstrap(sparse[0], b)


@pytest.mark.parametrize("case", F.cases(), ids=F.case_id)
def test_every_form_collects_the_same_bytes(case):
    results = {F.form_name(side, fused): F.run_form(case, side, fused) for side, fused in F.forms(case["head"])}
    _hold_together(results)
    if "masks" in case["feature"]:
        assert results["host" if case["head"] != "discrete" else "host-step"][1][0]["action_mask_words"] != b"none"
    if case["feature"] == "bootstrap" and case["n_agents"] == 16:   # (the agents IntegerEnv truncates: 6, 9, 12, 15)
        steps = results["host" if case["head"] != "discrete" else "host-chain"][1][1]["steps"]
        assert (steps % 9 != 8).any(), "the T = 9 collect must hold environment-side truncations, not the flush alone"
    if "critic" in case["feature"]:
        assert results["device" if case["head"] != "discrete" else "device-chain"][2][0]["critic_value_input_rows"] != b"none"


@pytest.mark.parametrize("side", ["host", "device"])
def test_fused_step_may_flip_between_collects(side):
    """policy.fused_step turned off between the second and the third collect: what carries over serves both heads' sides."""
    results = {"kept": F.run_form(F.FLIP_CASE, side, True), "flipped": F.run_form(F.FLIP_CASE, side, True, flip=True)}
    _hold_together(results)
