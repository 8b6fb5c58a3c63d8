"""dg_apply_deltas' one-pass fold (csrc/kfold.hip, kfold_pass in csrc/api_fold.hip) at its
bucket capacities, on skewed keys and at its other seams, bit-exact against the C oracle's
delta-by-delta fold (which tests/test_kfold_plan.py pins to the term oracle on these shapes).

Which path an input takes -- the first attempt, the retry with 8 T, refusal, which of the two
overflow sites -- cannot be seen from outside the library: the strict engine either answers
(one of the two one-pass attempts stood) or raises.  tests/kfold_plan.py models the host's
and the kernel's decisions, and tests/test_kfold_plan.py asserts for every input here that
the model sends it where this file says; each test names that reach assertion.  The tests
here then assert the model's verdict against the strict engine (so a capacity that moved by
one, or a missing retry, fails here) and the rows and the context against the oracle."""
import pytest

import kfold_plan as P
from delta_crdt_ex_amd._abi import DeltaGpuError
from kfold_cases import random_fold
from test_gpu_kfold import check, run, stepwise, strict  # noqa: F401 (the engines' fixtures)

pytestmark = pytest.mark.gpu

REFUSED = "one-pass fold not applicable"


def by_verdict(strict, engine, st, ds, verdict):
    """The strict engine folds what the model accepts; what it refuses, the strict engine
    refuses too and the default engine folds step by step."""
    assert P.verdict(st, ds) == verdict
    if verdict == "refuse":
        with pytest.raises(DeltaGpuError, match=REFUSED):
            run(strict, st, ds)
        check(engine, st, ds)
    else:
        check(strict, st, ds)


@pytest.mark.parametrize("layout", ["one", "many"])
def test_at_capacity(strict, layout):
    """Bucket 0 with exactly 1024 state rows, 512 delta rows, 1024 keyset entries (1536
    staged: threads 0..511 stage a second item) and 1024 items after the keyset fold: accepted
    at T0 = 2 (reach: test_kfold_plan.py::test_at_capacity_reach)."""
    st, ds = P.at_capacity(layout=layout)
    by_verdict(strict, None, st, ds, "first")


@pytest.mark.parametrize("layout", ["one", "many"])
@pytest.mark.parametrize("over", P.OVERS)
def test_over_capacity_refused(engine, strict, stepwise, over, layout):
    """One element over one capacity, packed so that bucket 0 of the retry holds it too:
    overflow twice, refused; "keep" overflows at the second site (after the keyset fold)
    both times.  The default engine and the step-by-step engine fold it
    (reach: test_kfold_plan.py::test_over_capacity_reach)."""
    st, ds = P.at_capacity(over, False, layout)
    by_verdict(strict, engine, st, ds, "refuse")
    check(stepwise, st, ds)


@pytest.mark.parametrize("layout", ["one", "many"])
@pytest.mark.parametrize("over", P.OVERS)
def test_over_capacity_retried(strict, over, layout):
    """The same one element over, spread so that 8 T0 fits: the fold the strict engine
    returns is the RETRY's, after a first attempt in which bucket 0 published an empty
    bucket from the first overflow site ("S", "D", "M") or the second ("keep")
    (reach: test_kfold_plan.py::test_over_capacity_reach).  With test_at_capacity and
    test_over_capacity_refused this pins every capacity exactly."""
    st, ds = P.at_capacity(over, True, layout)
    by_verdict(strict, None, st, ds, "retry")


@pytest.mark.parametrize("name", list(P.SKEW_CASES))
def test_rekeyed(engine, strict, name):
    """random_fold rekeyed to key sets that are not uniform hashes: refused where thousands
    of keys share bucket 0 at any T, the retry where a dense sixteenth / eighth overflows a
    bucket's STATE rows at T0 only, and at once where a small skewed set fits its bucket and
    the skew is inside it (reach: test_kfold_plan.py::test_rekeyed_reach,
    test_dense_part_overflows_on_state_rows, test_small_skewed_sets_sit_in_few_sub_buckets)."""
    st, ds = P.skew_case(name)
    by_verdict(strict, engine, st, ds, P.SKEW_CASES[name][5])


@pytest.mark.parametrize("gen", ["one_sub_bucket", "one_key_bucket", "ends", "all_runs_one_bucket",
                                 "gaps", "tiny_absent_keys"])
def test_inside_a_bucket(strict, gen):
    """one_sub_bucket: every element in one of the 1024 sub-buckets; one_key_bucket: one key
    holds 1024 state rows and 512 delta rows; ends: keys 0, 1, 2^64 - 2, 2^64 - 1;
    all_runs_one_bucket: k = 64 with all 128 runs in one bucket (bit 63 of every mask);
    gaps: the state in one bucket, runs empty over six buckets, buckets without state rows
    and one without items; tiny_absent_keys: T0 = 1 and a keyset of absent keys only
    (reach: test_kfold_plan.py::test_<gen>_reach)."""
    st, ds = getattr(P, gen)()
    by_verdict(strict, None, st, ds, "first")


@pytest.mark.parametrize("case", list(P.DOT_CASES))
def test_dot_edges(engine, strict, case):
    """Dot-set contexts at the packed key's limits: counter 2^48 - 2 and node 1023 are taken
    (and the dot found in the hash set), counter 2^48 - 1 and node 1024 refused by the prep;
    a probe sequence that wraps from slot 1023 to slot 0
    (reach: test_kfold_plan.py::test_dot_edges_reach, test_probe_wraps_the_table_end)."""
    st, ds, _ = P.dot_edges(case)
    by_verdict(strict, engine, st, ds, "refuse" if P.DOT_CASES[case] == "refuse" else "first")


def test_flagged_calls_leave_no_state_behind(strict):
    """On ONE engine: a call the prep refuses (KF_PREP_FAIL: no workgroup takes a ticket), a
    call that overflows twice (KF_OVERFLOW: every ticket taken, empty buckets published),
    then a good fold and a fold that needs the retry -- both right, and right again
    (reach: test_kfold_plan.py::test_hygiene_inputs_reach)."""
    prep, over = P.hygiene_inputs()
    good = [random_fold(0, n_keys=3000, k=1), P.at_capacity("keep", True, "many")]
    for bad in (prep, over):
        with pytest.raises(DeltaGpuError, match=REFUSED):
            run(strict, *bad)
    for _ in range(2):
        for st, ds in good:
            check(strict, st, ds)
    with pytest.raises(DeltaGpuError, match=REFUSED):
        run(strict, *over)
    check(strict, *good[1])


@pytest.mark.parametrize("case", ["second prep fails", "second overflows twice"])
def test_two_pass_fallback(engine, strict, case):
    """70 deltas whose first pass of 64 folds and whose second pass is refused (by the prep:
    node 1024 in delta 66's context; by two overflows: delta 65's keyset): the default engine
    starts over from the ORIGINAL state, step by step, while the first pass's result sits in
    the buffers that fold reuses (reach: test_kfold_plan.py::test_two_pass_reach)."""
    st, ds = P.two_pass(case)
    by_verdict(strict, engine, st, ds, "refuse")


def test_two_pass_first_pass_retries(strict):
    """70 deltas: the first pass overflows at T0 (keyset entries) and stands at 8 T0, the
    second pass stands at once (reach: test_kfold_plan.py::test_two_pass_reach)."""
    st, ds = P.two_pass("first retries")
    by_verdict(strict, None, st, ds, "retry")
