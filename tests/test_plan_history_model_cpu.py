"""tests/plan_history_model.py on sequences worked by hand (no GPU, no library).

Throughout: nt = 16 tiles per item, so an item is in exact mode on a run when
the count it left on the previous fast run is at least 3 (3 * 8 = 24 > 16) and
stays on the fast path at 2 (2 * 8 = 16, not greater).  Fast runs are numbered
from 0; run 15, 31 and 47 are probe runs."""
import pytest

from plan_history_model import PlanHistoryModel

NT = 16


def _fast(m, *U):
    return m.step('fast', list(U))


def test_item_enters_exact_mode_and_boundary_stays_fast():
    """Two items.  Run 0: U = (3, 2): both measured, count 5.
    Run 1: item 0 left 3 (24 > 16) -> exact, adds 16 whatever its content (U 0
    here); item 1 left 2 (16 == 16) -> fast, measures 0.  Count 16 + 0.
    Run 2: item 0 keeps 3 -> exact again; item 1 left 0 -> fast, measures 7.
    Count 16 + 7.  Run 3: item 1 left 7 -> both exact, count 32."""
    m = PlanHistoryModel(2, NT)
    s = _fast(m, 3, 2)
    assert (s.count, s.exact, s.prev, s.rot, s.parity, s.probe) == (5, (False, False), (0, 0), 0, 0, False)
    s = _fast(m, 0, 0)
    assert (s.count, s.exact, s.prev, s.rot, s.parity) == (16, (True, False), (3, 2), 1, 1)
    s = _fast(m, 0, 7)
    assert (s.count, s.exact, s.prev, s.rot, s.parity) == (23, (True, False), (3, 0), 2, 0)
    s = _fast(m, 0, 0)
    assert (s.count, s.exact, s.prev, s.rot) == (32, (True, True), (3, 7), 0)
    assert m.inv_runs == 4


def test_slot_rotation_zeroes_the_slot_after_next():
    """Run r writes slot r % 3 and zeroes slot (r + 1) % 3.  After runs 0, 1, 2
    with U = 1, 2, 1 the slots hold: run 0 -> [1, 0, 0]; run 1 -> [1, 2, 0];
    run 2 -> [0, 2, 1] (slot 0 zeroed for run 3)."""
    m = PlanHistoryModel(1, NT)
    _fast(m, 1)
    assert [s[0] for s in m.slots] == [1, 0, 0]
    _fast(m, 2)
    assert [s[0] for s in m.slots] == [1, 2, 0]
    _fast(m, 1)
    assert [s[0] for s in m.slots] == [0, 2, 1]


def test_exact_mode_holds_for_15_runs_whatever_the_content_then_probe_decides():
    """Run 0 measures U = 16 (flat content).  Runs 1..14 are exact whether the
    content stays flat (runs 1..7, U 16) or turns random (runs 8..14, U 0):
    count 16 each, the carried count stays 16.  Run 15 is the probe: it
    measures.  With fresh U = 2 (small) the item is released: run 16 is fast
    and counts its own U.  With fresh U = 3 it is not: run 16 is exact again.
    The next probe is run 31."""
    for fresh, released in ((2, True), (3, False), (0, True), (16, False)):
        m = PlanHistoryModel(1, NT)
        assert _fast(m, 16).count == 16
        for r in range(1, 15):
            s = _fast(m, 16 if r < 8 else 0)
            assert (s.count, s.exact, s.prev, s.probe) == (16, (True,), (16,), False), r
        s = _fast(m, fresh)
        assert (s.probe, s.exact, s.count, s.prev) == (True, (False,), fresh, (16,))
        s = _fast(m, 1)
        assert s.exact == (not released,) and s.count == (1 if released else 16)
        if not released:
            for r in range(17, 31):
                assert _fast(m, 0).exact == (True,), r
            s = _fast(m, 0)  # run 31
            assert (s.probe, s.exact, s.count) == (True, (False,), 0)
            assert _fast(m, 5).exact == (False,)


def test_probe_run_on_an_item_not_in_exact_mode_changes_nothing():
    """U = 1 on every run: runs 0..16 all fast, count 1, run 15 flagged probe."""
    m = PlanHistoryModel(1, NT)
    for r in range(17):
        s = _fast(m, 1)
        assert (s.count, s.exact, s.probe) == (1, (False,), r == 15), r


def test_seeded_item_is_first_measured_at_run_15():
    """A mixed plan: item 0 seeded (all three slots hold 16), item 1 not.
    Runs 0..14: item 0 exact (16), item 1 fast with U = 1: count 17.  Run 15
    (probe) measures item 0 for the first time: U = (4, 1) -> count 5.  Run 16:
    item 0 left 4 (32 > 16) -> exact again: count 16 + 1."""
    m = PlanHistoryModel(2, NT, seeded=[True, False])
    assert m.slots == [[16, 0], [16, 0], [16, 0]]
    for r in range(15):
        s = _fast(m, 0, 1)
        assert (s.count, s.exact) == (17, (True, False)), r
    s = _fast(m, 4, 1)
    assert (s.probe, s.exact, s.count) == (True, (False, False), 5)
    s = _fast(m, 0, 1)
    assert (s.exact, s.count, s.prev) == ((True, False), 17, (4, 1))


def test_fixall_pushes_every_item_into_exact_mode_on_the_next_run():
    """Run 0: U = (0, 1), count 1.  Run 1 is fix-all: every tile of both items,
    count 32, nobody in exact mode during it.  Run 2: both left 16 -> exact,
    count 32 (U ignored).  A fix-all run also overrides exact mode: run 3 as
    fix-all has exact = (False, False) and count 32 again."""
    m = PlanHistoryModel(2, NT)
    assert _fast(m, 0, 1).count == 1
    s = m.step('fast_fixall')
    assert (s.count, s.exact) == (32, (False, False))
    s = _fast(m, 0, 0)
    assert (s.count, s.exact, s.prev) == (32, (True, True), (16, 16))
    s = m.step('fast_fixall')
    assert (s.count, s.exact) == (32, (False, False))


def test_exact_and_forward_only_runs_advance_no_cycle():
    """Run 0 (fast): U = 3, count 3.  A forward-only run reports the same 3
    (the fast inverse's counter is still live).  An exact-inverse run reports 0,
    and a forward-only run after it reports 0 too.  None of them moved
    inv_runs: the next fast run is run 1 (rot 1, parity 1), reads the 3 run 0
    left and is exact.  Fourteen exact-inverse runs later the probe is still the
    16th *fast* run."""
    m = PlanHistoryModel(1, NT)
    assert _fast(m, 3).count == 3
    assert m.step('fwd_only').count == 3
    assert m.step('exact_inv').count == 0
    assert m.step('fwd_only').count == 0
    assert m.inv_runs == 1
    s = _fast(m, 0)
    assert (s.rot, s.parity, s.exact, s.count, s.prev) == (1, 1, (True,), 16, (3,))
    assert m.step('fwd_only').count == 16
    for r in range(2, 15):
        m.step('exact_inv')
        s = _fast(m, 0)
        assert (s.probe, s.exact) == (False, (True,)), r
    m.step('exact_inv')
    s = _fast(m, 0)  # fast run 15
    assert (s.probe, s.exact, s.count) == (True, (False,), 0)


def test_non_adaptive_kernels_rotate_but_never_enter_exact_mode():
    """k_inv_fast444 / k_inv16_fast: U = 16 on every run, count 16 from
    measuring, never from exact mode; the slots still rotate."""
    m = PlanHistoryModel(1, NT, adaptive=False)
    for r in range(20):
        s = _fast(m, 16 if r % 2 == 0 else 1)
        assert s.exact == (False,) and s.count == (16 if r % 2 == 0 else 1)
        assert s.prev == ((0,) if r == 0 else (1,) if r % 2 == 0 else (16,))


def test_bad_arguments_are_rejected():
    m = PlanHistoryModel(2, NT)
    with pytest.raises(AssertionError):
        m.step('fast', [1])
    with pytest.raises(AssertionError):
        m.step('fast', [17, 0])
    with pytest.raises(AssertionError):
        m.step('inverse', [0, 0])
