"""Host side of "nep_iar_run without a history buffer": the one decision of the Python host (iar._native_run_keeps_history) over
every combination of its inputs, and the batch planner, which the rule leaves as it is (csrc/iar_run.hip feeds it the one check
step m instead of all of them; the formula is untouched)."""
import itertools
import sys

import numpy as np
import pytest

import nep_amd as na

iar_mod = sys.modules["nep_amd.iar"]


@pytest.mark.parametrize("errhist,neigs,logger", list(itertools.product([None, []], [6, np.inf], [0, 1])))
def test_the_buffer_is_left_out_exactly_when_nobody_reads_it(errhist, neigs, logger):
    keep = iar_mod._native_run_keeps_history(errhist, neigs, logger)
    assert keep is not (errhist is None and neigs == np.inf and logger == 0)


def test_other_spellings_of_the_inputs():
    f = iar_mod._native_run_keeps_history
    assert not f(None, float("inf"), 0) and not f(None, np.float64(np.inf), False)
    assert f(None, -np.inf, 0)                      # not "run to maxit": the stop test fires at once
    assert f(None, 10 ** 6, 0) and f(None, np.inf, 2) and f([1.0], np.inf, 0)


def test_the_binding_knows_the_new_entry_points():
    for name in ("nep_iar_run_stats", "nep_iar_ready", "nep_iar_event_mask"):
        assert name in na._lib.SIGNATURES and hasattr(na._lib.lib, name)


def test_batch_plan_is_unchanged():
    """the planner's answers for the headline shapes, written down before the change"""
    plan = iar_mod._eig_batch_plan
    assert sorted(plan(100, 1, 16, 8, 3.3)) == list(range(1, 24)) + [25, 27, 29, 31, 34, 37, 41, 45, 50, 57, 65, 76, 92, 100]
    assert sorted(plan(40, 3, 16, 8, 3.3)) == [3, 6, 9, 12, 15, 18, 40]
    assert sorted(plan(100, 100, 16, 8, 3.3)) == [100]          # the one check step of a run without history
