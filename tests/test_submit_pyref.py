"""tests/submit_pyref.py (the truth the device is held to) against the hand-derived table of tests/submit_case.py: codes, rewritten time
limits, the counters and the exists bits after the batch, all written out by hand from the cited lines."""
import numpy as np
import pytest

from cranesched_amd import abi

from tests import submit_case as sc
from tests import submit_pyref as sp


@pytest.fixture(scope="module")
def hand():
    return sc.hand_table()


def test_hand_table_codes_and_time_limits(hand):
    t, jobs, keys, codes, tlo, admitted, created = hand
    got_code, got_tlo, got_adm, _ = sp.run(t, jobs, keys)
    for j in range(jobs.num_jobs):
        assert got_code[j] == codes[j], f"job {j}: {abi.SUBMIT_STR[int(got_code[j])]}, by hand {abi.SUBMIT_STR[int(codes[j])]}"
    assert np.array_equal(got_tlo, tlo)
    assert got_adm == len(admitted) == 8


def test_hand_table_holds_every_code_once(hand):
    assert set(int(c) for c in hand[3]) == set(range(17)) == set(abi.SUBMIT_STR)


def test_hand_table_state_after_the_batch(hand):
    t, jobs, keys, codes, tlo, admitted, created = hand
    state = sp.run(t, jobs, keys)[3]
    want = sc.expected_state(t, admitted, created)
    for f in want.__dataclass_fields__:
        assert np.array_equal(getattr(state, f), getattr(want, f)), f
    Q, Pn = t.num_qos, t.num_partitions
    # by hand once more, the records most of the table shares: account 8 x partition 0 got 2 + 2 + 1 + 1 + 1 + 1, QoS 0 got 1 + 3
    assert state.acct_part_submit[8 * Pn + 0] == 8 and state.qos_submit[0] == 4 and state.user_qos_submit[15 * Q + 10] == 21
    # skip, count == 0 and every rejected job add nothing: the root of the six-account chain is as it was, its leaf untouched
    assert state.acct_qos_submit[2 * Q + 12] == 4 and state.acct_qos_submit[7 * Q + 12] == 0 and state.user_qos_submit[0 * Q + 0] == 3
    assert state.user_exists[17] == 1 and state.qos_exists[3] == 1
    assert t.user_exists[17] == 0 and t.qos_exists[3] == 0      # the tables themselves are inputs and stay


def test_hand_table_on_a_wide_layout():
    """CheckGres_'s walk order where class index and name disagree (tests/gres_wide.py, eight_by_8_four_names)."""
    t, jobs, keys, codes = sc.hand_table_wide()
    got_code, got_tlo, got_adm, _ = sp.run(t, jobs, keys)
    for j in range(jobs.num_jobs):
        assert got_code[j] == codes[j], f"job {j}: {abi.SUBMIT_STR[int(got_code[j])]}, by hand {abi.SUBMIT_STR[int(codes[j])]}"
    assert jobs.num_jobs >= 8 and got_adm == int((codes == 0).sum()) == 5 and np.array_equal(got_tlo, jobs.time_limit_sec)
    # rows 4 and 5 are the ones a walk in class-index order gets wrong: on the layout with class_name sorted (where the two orders
    # coincide, and classes 0, 1 share a name) the restatement itself answers the other way
    from tests import gres_wide as gw
    other = sp.run(gw.with_sorted_class_names(t), jobs, keys)[0]
    assert other[4] != codes[4] and other[5] != codes[5]


def test_carry_equals_one_batch(hand):
    t, jobs, keys = hand[0], hand[1], hand[2]
    from cranesched_amd import submit as sb
    whole = sp.run(t, jobs, keys)
    h = jobs.num_jobs // 2
    a = sp.run(t, sb.slice_jobs(jobs, 0, h), keys.slice(0, h))
    b = sp.run(t, sb.slice_jobs(jobs, h, jobs.num_jobs), keys.slice(h, jobs.num_jobs), state=a[3])
    assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0]) and a[2] + b[2] == whole[2] and b[3].same_as(whole[3])


def test_input_rules():
    t, jobs, keys = sc.random_case(1, 50)
    keys.qos[7] = t.num_qos
    keys.skip[7] = 0
    with pytest.raises(sp.Refused) as e:
        sp.run(t, jobs, keys)
    assert e.value.status == sp.ERR_INVALID_ARG
    keys.skip[7] = 1                                            # a skipped job is not read
    sp.run(t, jobs, keys)
    t.qos_submit[0] = 0xFFFFFFFF - 10
    keys.count[:] = 1
    with pytest.raises(sp.Refused) as e:
        sp.run(t, jobs, keys)
    assert e.value.status == sp.ERR_UNSUPPORTED
