"""The stage instrument (tests/stage_checks.py) on the CPU: the evaluator equals the oracle, the NumPy float32 stand-in passes every
case of the GPU module's list at half a bar with bounds that are not slack, the restated dispatch and skip count are right at every
threshold, and every wrong device fails a case.  tests/test_gpu_stages.py drives the same code with the kernels."""
import numpy as np
import pytest

from oracle import OracleSimulator

import stage_checks as S

# the case a wrong device is expected to fail first (any other case of the list may fail too; a mutant no case fails is an error)
FAILS_AT = {"carry-row": "scans-B7-", "no-src-prev": "scans-B7-", "prev-product-skipped": "zero-", "zero-map-kept": "zero-",
            "inc-skipped-as-set": "zero-", "memset-wide": "zero-", "k-tail": "products-B33-", "tile-edge": "products-B33-",
            "chunk-power": "scans-B257-", "multi-tail": "chain-B13-", "op-25": "elementwise-B8-", "coefficient": "scans-B64-100",
            "probe-early": "probes-B64-", "scan-tail": "scans-B9-"}


@pytest.fixture(scope="module")
def standin_runs():
    """Every case on the stand-in -> [(case, failures, worst ratio)], and the pooled bar / error figures per operator kind."""
    tight, runs = {}, []
    for case in S.CASES:
        dev = S.run_case(case, S.StandIn(case.model, case.block))
        fails, worst = S.failures_of(case, dev, tight=tight)
        runs.append((case, fails, worst))
    return runs, tight


def test_the_evaluator_equals_the_oracle():
    """``evaluate`` walks the operators in ``border`` order, all timesteps at once; ``OracleSimulator`` steps them in step order - the
    delayed product of the zero model included."""
    for built, steps in ((S.products_model, 120), (S.the_scans_model, 150), (S.elementwise_model, 20), (S.chain_model, 20), (S.zero_model, 300),
                         (S.probes_model, 60)):
        model = built().model
        ref = OracleSimulator(model)
        ref.run_steps(steps)
        ev = S.evaluate(model, steps)
        for i, p in enumerate(model.probes):
            if p["every"] == 1:
                np.testing.assert_allclose(ref.probe_data(i), ev.V[1:, p["src"]:p["src"] + p["width"]], atol=1e-12, rtol=0)
    z = S.zero_model()
    ev = S.evaluate(z.model, 300)
    d = z.model.probes[z.probes["delayed"]]
    assert np.abs(ev.V[129, d["src"]:d["src"] + d["width"]]).max() > 0.05 and not z.tables["e"].stored(range(129, 193)).any()
    assert not ev.V[130:, d["src"]:d["src"] + d["width"]].any()


def test_the_standin_passes_every_case_at_half_a_bar(standin_runs):
    runs, _ = standin_runs
    for case, fails, worst in runs:
        print("%-32s worst %.3f of the bar" % (case.id, worst))
    assert not [(c.id, f) for c, f, w in runs if f]
    assert max(w for _, _, w in runs) <= 0.5


def test_the_bounds_are_not_slack(standin_runs):
    """bar / |NumPy f32 - float64|, median over the elements the f32 run did not get exactly, per operator kind, pooled over the case
    list: at most 64 (the condition of tests/test_slam_restart.py)."""
    t = S.tightness(standin_runs[1])
    print({k: round(v, 1) for k, v in t.items()})
    assert {"matvec", "lowpass", "axpy"} <= set(t)
    for kind, v in t.items():
        assert v <= 64.0, (kind, v)


def test_the_chunked_bound_follows_the_kernels_arithmetic():
    """The chunked recursion bounds another algorithm than the sequential one (the chunk's own run starts from zero, so its terms are
    those of z, not of y; the carries add theirs): neither dominates element by element, the values are the same, and over a run the
    two stay within a few per cent of each other - the term is the kernel's arithmetic, not room."""
    case = [c for c in S.CASES if c.id.startswith("scans-B257-")][0]
    seq, chk = S.evaluate(case.model, case.steps), S.evaluation(case)
    lp = chk.kind == "lowpass"
    assert np.array_equal(seq.V, chk.V) and lp.any()
    assert (chk.B[1:, lp] != seq.B[1:, lp]).any() and np.array_equal(chk.B[:, ~lp & (chk.kind != "matvec")], seq.B[:, ~lp & (chk.kind != "matvec")])
    ratio = chk.B[1:, lp].sum() / seq.B[1:, lp].sum()
    print("chunked / sequential bound, summed over the run: %.4f" % ratio)
    assert 0.9 <= ratio <= 1.25


def test_the_restated_dispatch_at_every_threshold():
    M, G, C, L, E = "kb_gemm_mfma_f32", "kb_gemm", "kb_lowpass_chunked", "kb_lowpass", "kb_elementwise"
    for kind in (S.K_MATVEC_INC, S.K_MATVEC_SET):
        assert S.dispatch(kind, 32, 64, 32) == M
        assert S.dispatch(kind, 31, 64, 32) == G and S.dispatch(kind, 32, 63, 32) == G and S.dispatch(kind, 32, 64, 31) == G
        assert S.dispatch(kind, 150, 129, 100) == M and S.dispatch(kind, 150, 129, 100, f32=False) == G
    assert S.dispatch(S.K_LOWPASS, 1, 0, 256) == C and S.dispatch(S.K_LOWPASS, 1, 0, 255) == L
    assert S.dispatch(S.K_LOWPASS, 65, 0, 1000, f32=False) == L
    assert S.dispatch(S.K_FILL, 5, 0, 7) == E and S.dispatch(S.K_FILL, 0, 0, 7) is None and S.dispatch(S.K_LOWPASS, 5, 0, 0) is None
    # the product sweep crosses every threshold from both sides with the other two conditions met, and reaches both kernels at tiles
    # that are ragged in all three dimensions
    ops = S.optimise(S.batch_ops(S.products_model().model))
    got = S.reached(S.plan_key(ops), S.PRODUCT_BLOCKS)
    for lo, hi in (((33, 63, 33), (33, 64, 33)), ((31, 65, 33), (32, 65, 33)), ((33, 64, 31), (33, 64, 32)), ((150, 100, 31), (150, 100, 32))):
        assert lo in got[G] and hi in got[M], (lo, hi)
    assert any(r % 64 and c % 32 and B % 64 for r, c, B in got[M]) and any(r % 32 and c % 32 and B % 32 for r, c, B in got[G])


def test_the_derived_skip_count_on_hand_made_windows():
    z = np.zeros((10, 2))
    early, late, never = S.Rows(np.ones((3, 2)), first=1), S.Rows(np.ones((2, 2)), first=9), S.Rows(z)
    stored = S.StoredRows(z)
    assert S.expected_skips([early], [4, 4, 2]) == 2 and S.expected_skips([late], [4, 4, 2]) == 2      # steps 1 .. 3: block 0; 9, 10: block 2
    assert S.expected_skips([late], [8, 2]) == 1 and S.expected_skips([late], [10]) == 0
    assert S.expected_skips([never], [4, 4, 2]) == 3 and S.expected_skips([stored], [4, 4, 2]) == 0
    assert S.expected_skips([early, early, late, never, stored], [4, 4, 2]) == 2 + 2 + 2 + 3
    assert S.cuts_of(64, S.UNEVEN) == [64, 36, 1, 64, 64, 64, 7] and S.cuts_of(64, (300,)) == [64, 64, 64, 64, 44]
    zm = S.zero_model()
    assert S.expected_skips(zm.skippable, S.cuts_of(64, (300,))) == 14      # a: blocks 0, 2, 4 x 2 products; b: blocks 0, 2, 3, 4 x 2


def test_the_packing_of_the_elementwise_model():
    """What the element-wise cases claim to reach, from the restated plan (which the GPU tests hold to the library's listing): a list
    that overflows, operators of different lengths in one list, a reset that is kept whole beyond 32 pieces, a chain of reset / sums /
    hand-off in one list and a previous-row read that opens another."""
    model = S.elementwise_model().model
    raw = S.batch_ops(model)
    ops = S.optimise(raw)
    launches = S.pack(ops)
    lists = [item for what, item in launches if what == "list"]
    assert any(len(l) == S.MAX_BATCH_OPS for l in lists) and any(len({o["len"] for o in l}) > 2 for l in lists)
    fills = [o for o in raw if o["kind"] == S.K_FILL]
    assert any(o["kind"] == S.K_FILL and o["len"] == max(f["len"] for f in fills) and o["len"] > 32 for o in ops)      # kept whole
    assert len(S.pack(ops, stage_batch=False)) == len(ops)
    chain = S.chain_model()
    ops = S.optimise(S.batch_ops(chain.model))
    s = chain.model.probes[chain.probes["sum"]]["src"]
    on_sum = lambda o: (o["dst"] == s and o["kind"] in S.WRITES) or (o["src"] == s and o["kind"] == S.K_AXPY_INC)
    lists = [item for what, item in S.pack(ops) if what == "list"]
    one = [l for l in lists if [o["kind"] for o in l if on_sum(o)] == [S.K_FILL, S.K_AXPY_INC, S.K_AXPY_INC, S.K_AXPY_INC]]
    assert one, [[o["kind"] for o in l] for l in lists]                  # reset, two sums, hand-off: one launch
    assert all(S.hazard(a, b) == 1 for l in one for i, a in enumerate(l) for b in l[i + 1:] if on_sum(a) and on_sum(b))
    prev = [o for o in ops if o["prev"]]
    assert len(prev) == 1 and prev[0]["kind"] == S.K_AXPY_INC
    assert not any(prev[0] in l for l in one)                                   # the previous-row read is another launch


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_every_wrong_device_fails_a_case(mutant):
    assert len(S.MUTANTS) >= 12
    first = [c for c in S.CASES if c.id.startswith(FAILS_AT[mutant])]
    assert first, FAILS_AT[mutant]
    for case in first + [c for c in S.CASES if c not in first and c.steps <= 700]:
        fails, worst = S.failures_of(case, S.run_case(case, S.StandIn(case.model, case.block, mutant=mutant)))
        if fails:
            print("%s fails %s: %s" % (mutant, case.id, fails[:2]))
            assert case in first, "expected to fail %s first" % FAILS_AT[mutant]
            return
    pytest.fail("no case of the list notices the wrong device %r" % mutant)
