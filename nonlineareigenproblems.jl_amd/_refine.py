"""Iterative refinement after a factorised solve: UMFPACK's stopping rule (umfpack_solve's refinement loop behind `Afact \\ x`,
src/LinSolvers.jl:114-122) as ONE function, and the per-solver policy object that applies it -- the Python twin of `struct Refine`
in csrc/iar_run.hip, which holds the same rule for nep_iar_run (tests/test_host_logic.py keeps the two equal)."""
import numpy as np

from ._env import env_str

EPS = np.finfo(float).eps

GO, STOP, TAKE_BACK = 0, 1, 2


def rule_step(omega, w_prev, step, umf):
    """the rule's decision on x_step, whose backward error is omega (w_prev: that of x_{step-1}, inf for x_0): GO = take another
    sweep, STOP = return x_step, TAKE_BACK = return x_{step-1}.  Stops after `umf` sweeps at the latest."""
    if omega <= 2.0 * EPS:                       # UMFPACK: omega < eps.  The computed omega carries round-off of
        return STOP                              # its own; a step taken at (eps, 2 eps] cannot halve it
    if omega > 0.5 * w_prev:
        return TAKE_BACK if omega > w_prev else STOP      # the last step made it worse: take it back
    return STOP if step == umf else GO


class Refine:
    """What one FactorizeLinSolver knows about the refinement of its solves: how many sweeps a solve takes without reading
    omega back, and the verdict of the rule on what such a solve recorded.  `nep` (may be None: no hint kept) carries the hint,
    the count a previous solver of the same NEP settled on at the same shift, as nep._refine_hint / _refine_hint_lam /
    _refine_hint_off; it is reached through this class only."""

    def __init__(self, umfpack_refinements, nep=None, lam=None):
        self.umf = umfpack_refinements
        self.nep = nep
        self.lam = None if lam is None else complex(lam)
        self.recorded = None            # sweeps the stopping rule asked for on the last reviewed record (nep_iar_step)
        self.last_omega = None
        self._plan = 0                  # refinement steps the last checked solve needed
        self._stable = 0                # consecutive checked solves that needed exactly _plan steps
        self.solves = 0
        self.refine_steps_taken = 0
        self.refine_checks = 0

    # ---- solves that record omega of every iterate and are reviewed afterwards (nep_iar_step, nep_iar_run)

    def plan(self):
        """refinement sweeps of the next solve of a step that RECORDS omega of every iterate (nep_iar_step): the settled
        count once a record has been reviewed, the maximum before"""
        if self.umf <= 0:
            return 0
        # the record holds omega of x_0..x_3; two sweeps to start with (gun needs one), a rule that asks for more is a miss.
        # A solver of a NEP whose previous solver settled on a count starts with that count (nep._refine_hint: iar issues
        # all its steps before the first record is reviewed, so without the hint every step of every run takes the two
        # sweeps; gun: omega(x_1) <= 1.7 eps in every step of every run, one sweep, 46 us less per step); a wrong hint is a
        # miss like any other, and a miss withdraws it.  NEP_REFINE_HINT=0 turns it off.
        if self.recorded is not None:
            return self.recorded
        hint = self.hint()
        return min(self.umf, 2 if hint is None else hint)

    def settled(self):
        """True when the refinement count of this solver's NEP has settled (a reviewed record of this solver, or the count a
        previous solver of the NEP settled on): steps may then skip the record of the kept iterate 7 times out of 8"""
        return self.recorded is not None or self.hint() is not None

    def hint(self):
        """the sweep count a previous solver of this NEP settled on AT THIS SHIFT (None otherwise): conditioning and pivot growth
        of M(sigma) change with sigma, so a count learnt at another shift says nothing about this factorisation"""
        if env_str("NEP_REFINE_HINT", "1") == "0":
            return None
        h = getattr(self.nep, "_refine_hint", None)
        if h is None or getattr(self.nep, "_refine_hint_lam", None) != self.lam:
            return None
        return h

    def note_hint(self, plan):
        """plan = None: a miss -- the hint is withdrawn for good on this NEP object (a problem whose omega sits at the edge of the
        rule would otherwise alternate between learning the count and missing with it, every miss a re-run of the call)"""
        nep = self.nep
        if nep is not None:
            try:
                if plan is None:
                    nep._refine_hint = None
                    nep._refine_hint_off = True
                elif not getattr(nep, "_refine_hint_off", False):
                    nep._refine_hint = plan
                    nep._refine_hint_lam = self.lam
            except AttributeError:
                pass

    def native_run(self, opts, res, call):
        """the refinement side of one nep_iar_run: the count the run starts with goes into opts.refine_hint (-1: none), call()
        makes the run, and what the run learnt (res.refine_plan / res.refine_hint_off of its nep_iar_result) belongs to this
        NEP and shift like a record reviewed here.  Returns what call() returned."""
        hint = self.recorded if self.recorded is not None else self.hint()
        opts.refine_hint = -1 if hint is None else int(hint)
        st = call()
        if res.refine_hint_off:
            self.note_hint(None)
        elif res.refine_plan >= 0 and self.umf > 0:
            self.recorded = int(res.refine_plan)
            self.note_hint(self.recorded)
        return st

    def review(self, w, plan, final_recorded=True):
        """UMFPACK's stopping rule (the loop of FactorizeLinSolver.solve_dev) replayed on the recorded omegas w[0..plan] of a solve
        that took `plan` sweeps without looking.  True: what was returned is what the checked loop returns, or an iterate at least as
        good; False: the checked loop would have continued, or would have taken a worsening sweep back.
        final_recorded=False: omega of the kept iterate x_plan was not evaluated (a step that took it on trust, 7 of 8 once
        the count has settled); the rule is replayed on x_0..x_{plan-1} and must not have stopped there."""
        if not final_recorded:
            w_prev = np.inf
            for step in range(plan):
                omega = float(w[step])
                if np.isfinite(omega) and omega <= 2.0 * EPS:
                    # the checked loop would have stopped at x_step, which satisfies UMFPACK's criterion already; the sweeps taken
                    # beyond it start from a converged iterate (a sweep from there moves x by O(eps) |x|): accepted, and the
                    # following steps plan that many sweeps -- not a miss (a miss re-runs the whole call unfused)
                    self.recorded = max(step, 1)
                    return True
                if not np.isfinite(omega) or omega > 0.5 * w_prev:
                    self.note_hint(None)           # the checked loop would have stopped before the sweeps that were taken
                    return False
                w_prev = omega
            return True
        w = [float(x) for x in w[:plan + 1]]
        w_prev = np.inf
        for step in range(self.umf + 1):           # (rule_step stops at step == umf at the latest: ret is always set)
            if step > plan:
                # the rule would go on.  At the noise level of omega itself (its own evaluation carries a few eps of
                # round-off: 4.49e-16 observed on gun against the 4.44e-16 threshold) a further sweep cannot improve the
                # iterate -- accepted; anything larger is a miss
                if np.isfinite(w[plan]) and w[plan] <= 4.0 * EPS:
                    ret = plan
                    break
                self.note_hint(None)
                return False
            verdict = rule_step(w[step], w_prev, step, self.umf)
            if verdict != GO:
                ret = step - 1 if verdict == TAKE_BACK else step
                break
            w_prev = w[step]
        self.last_omega = w[plan]
        # never plan fewer than one sweep: the accuracy of the raw solve changes within a run when the dense apex of the
        # block schedule comes on line (trsv_ml.hip: built behind the first solves), and a plan of 0 learnt before would
        # turn the first solve after it into a miss (a full re-run of the call)
        self.recorded = max(ret, 1)
        ok = bool(np.isfinite(w[plan]) and (ret == plan or w[plan] <= max(4.0 * EPS, w[ret])))
        self.note_hint(self.recorded if ok else None)
        return ok

    def note_blind_solve(self, plan):
        self.solves += 1
        self.refine_steps_taken += plan

    # ---- solves whose loop reads omega back (FactorizeLinSolver.solve_dev)

    def next_solve(self):
        """counts a solve and says how it refines: the number of sweeps to take on trust (0: none at all), or None for a solve
        that evaluates omega after every sweep.  Every evaluation of omega is a host synchronisation.  Once 4 consecutive
        checked solves needed the same number of steps (same factors, same conditioning), 7 of 8 solves take that many steps
        blindly."""
        self.solves += 1
        if self.umf <= 0:
            return 0
        return self._plan if (self._stable >= 4 and (self.solves % 8) != 0) else None

    def checked_solve(self, steps, omega):
        """a checked solve took `steps` sweeps and kept an iterate with backward error omega"""
        self.refine_checks += 1
        self.last_omega = omega
        self.refine_steps_taken += steps
        if steps == self._plan:
            self._stable += 1
        else:
            self._plan, self._stable = steps, 0
