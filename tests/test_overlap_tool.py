"""CPU: the interval bookkeeping of tools/overlap.py (who runs beside whom in a kernel trace) on traces small enough to check by hand, and
the null-context answer of afv_set_split_schedule."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("afv_overlap_tool", os.path.join(ROOT, "tools", "overlap.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_same_other_alone_add_up_to_the_launch_durations():
    ov = _tool()
    #  k_a: [0, 10) and [5, 15): 5 .. 10 beside its twin (both launches count), 0 .. 5 and 10 .. 12 alone, 12 .. 15 beside k_b
    #  k_b: [12, 20): 12 .. 15 beside k_a, 15 .. 20 alone; [30, 40) alone
    res = ov.classify([(0, 10, "k_a"), (5, 15, "k_a"), (12, 20, "k_b"), (30, 40, "k_b")])
    assert res == {"k_a": [2, 10, 3, 7], "k_b": [2, 0, 3, 15]}
    assert sum(res["k_a"][1:]) == 10 + 10 and sum(res["k_b"][1:]) == 8 + 10   # the summed durations of the launches


def test_back_to_back_launches_do_not_overlap_and_twins_beside_a_third_count_as_same():
    ov = _tool()
    assert ov.classify([(0, 10, "k_a"), (10, 20, "k_a")]) == {"k_a": [2, 0, 0, 20]}
    res = ov.classify([(0, 10, "k_a"), (0, 10, "k_a"), (0, 10, "k_b")])
    assert res == {"k_a": [2, 20, 0, 0], "k_b": [1, 0, 10, 0]}


def test_summary_is_per_step():
    ov = _tool()
    s = ov.summarise([(0, 1000000, "k_a"), (500000, 2000000, "k_b")], 2)
    assert s["wall_ms_per_step"] == 1.0
    assert s["kernels"]["k_a"]["other_ms_per_step"] == 0.25 and s["kernels"]["k_a"]["alone_ms_per_step"] == 0.25
    assert s["kernels"]["k_b"]["same_frac"] == 0.0


def test_split_schedule_needs_a_context(afv):
    assert afv._lib.load().afv_set_split_schedule(None, 1) == afv._lib.EINVAL
