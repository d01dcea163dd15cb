"""Host model of a jds_plan's run-history counters (pure Python, no library).

Restates csrc/jds_internal.hpp (InvFix), jds_plan::inv_fix() and jds_plan_run /
jds_plan_fix_counts of csrc/jds_abi.hip:

* `inv_runs` counts the runs whose inverse was the certified fast kernel.  It
  alone drives the three cycles: parity = inv_runs % 2 (which run counter a run
  counts into; it zeroes the other), rot = inv_runs % 3 (which per-item slot it
  writes; it reads slot (rot + 2) % 3 and zeroes slot (rot + 1) % 3) and
  probe = inv_runs % 16 == 15.
* `slots[3][n]`: tiles of item i the exact tile code recomputed, per rotation
  slot.  All zero at creation, except that a mixed plan (some tables coarse,
  some not) seeds its coarse items with `nt` in all three slots.
* On the adaptive kernels (k_inv_fast, 4:2:0 and 4:2:2) an item whose previous
  run recomputed more than 1/8 of its tiles (prev * 8 > nt) runs the exact tile
  code directly, keeps its count and adds all `nt` tiles to the run count;
  a probe run and a fix-all run measure every item afresh.  k_inv_fast444 and
  k_inv16_fast rotate and zero the slots but have no exact mode.
* Runs whose inverse is an exact kernel, and forward-only runs, leave all of
  this alone.  jds_plan_fix_counts()[1] is the last run's count while the last
  inverse was the fast one (a forward-only run does not change that), else 0.

`U[i]` is what item i's content measures on the fast path: the tiles that fail
the certificate (the caller measures it on a fresh plan)."""
from collections import namedtuple

KINDS = ('fast', 'fast_fixall', 'exact_inv', 'fwd_only')

# count: the expected fix_counts()[1] after the run.  For fast runs also the
# cycle positions the run used, per item the previous run's count it read, and
# whether the item ran in exact mode; None / empty for the other kinds.
Step = namedtuple('Step', 'count kind rot parity probe prev exact')


class PlanHistoryModel:
    def __init__(self, n, nt, adaptive=True, seeded=None):
        """n items of nt inverse tiles each; seeded[i]: the item starts in exact mode."""
        self.n, self.nt, self.adaptive = int(n), int(nt), bool(adaptive)
        seeded = [False] * self.n if seeded is None else [bool(s) for s in seeded]
        assert len(seeded) == self.n
        self.inv_runs = 0
        self.slots = [[self.nt if s else 0 for s in seeded] for _ in range(3)]
        self.last_inv_fast = False
        self.last_fast_count = 0

    def step(self, kind, U=None):
        assert kind in KINDS, kind
        if kind == 'fwd_only':  # last_inv_fast and the live run counter stay as they are
            return Step(self.last_fast_count if self.last_inv_fast else 0, kind, None, None, None, (), ())
        if kind == 'exact_inv':
            self.last_inv_fast = False
            return Step(0, kind, None, None, None, (), ())
        fixall = kind == 'fast_fixall'
        U = [self.nt] * self.n if fixall else [int(u) for u in U]
        assert len(U) == self.n and all(0 <= u <= self.nt for u in U), U
        rot, parity, probe = self.inv_runs % 3, self.inv_runs % 2, self.inv_runs % 16 == 15
        prev = tuple(self.slots[(rot + 2) % 3])
        exact = tuple(self.adaptive and not probe and not fixall and prev[i] * 8 > self.nt for i in range(self.n))
        count = 0
        for i in range(self.n):
            self.slots[rot][i] = prev[i] if exact[i] else U[i]
            self.slots[(rot + 1) % 3][i] = 0
            count += self.nt if exact[i] else U[i]
        self.inv_runs += 1
        self.last_inv_fast = True
        self.last_fast_count = count
        return Step(count, kind, rot, parity, probe, prev, exact)
