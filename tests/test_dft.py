"""The transform tests without a GPU: the instrument of tests/dft_checks.py.  The float64 matrices the oracle multiplies by are a DFT
(np.fft), ``dft_structure`` names them and nothing else, the restated planner reaches what the sweep claims, the float32 stand-in of
the three engines stays under half a bar and the bars under their analytic worst case, and every wrong device fails."""
import numpy as np
import pytest

import dft_checks as D
from sspslam_amd.builder import build, dft_structure
from sspslam_amd.networks.binding import transform_in, transform_out
from oracle import OracleSimulator


# -- the reference ------------------------------------------------------------------------------------------------------------
def test_the_matrices_are_a_dft():
    """Every d in 8..256: the four slots of ``transform_in`` against ``np.fft.rfft`` (and its conjugate), ``transform_out`` against
    ``np.fft.irfft`` of (s0 - s1) + i (s2 + s3), to 1e-12 - independent of the package's own ``dft_half``."""
    rng = np.random.RandomState(3)
    for d in D.SWEEP:
        H = d // 2 + 1
        x = rng.randn(3, d)
        F = np.fft.rfft(x, axis=1)
        for kind, (align, inv) in D.KIND_OF.items():
            G = F.conj() if inv else F
            got = (x @ transform_in(d, align, inv).T).reshape(3, H, 4)
            want = np.stack([G.real, G.imag, G.imag if align == "B" else G.real, G.real if align == "B" else G.imag], axis=2)
            assert np.abs(got - want).max() <= 1e-12 * np.abs(x).sum(axis=1).max(), (d, kind)
        s = rng.randn(3, H, 4)
        Y = (s[:, :, 0] - s[:, :, 1]) + 1j * (s[:, :, 2] + s[:, :, 3])
        got = s.reshape(3, 4 * H) @ transform_out(d).T
        assert np.abs(got - np.fft.irfft(Y, n=d, axis=1)).max() <= 1e-12, d


def test_dft_structure_names_the_five_maps_and_nothing_else():
    for d in range(8, 301):
        assert [dft_structure(D.matrix(d, k)) for k in (1, 2, 3, 4, 5)] == [1, 2, 3, 4, 5], d
    for d in (4, 7):
        assert dft_structure(transform_in(d, "A", False)) == 0 and dft_structure(transform_out(d)) == 0
    for d in (8, 45, 74):
        for k in (1, 2, 3, 4, 5):
            T = D.matrix(d, k)
            moved = T.copy()
            moved[3, 5] += 1e-9
            near = T + np.random.RandomState(d).uniform(-9e-13, 9e-13, T.shape)
            assert dft_structure(0.5 * T) == 0 and dft_structure(moved) == 0 and dft_structure(near) == k
            assert dft_structure(np.ascontiguousarray(T.T)) == 0 and dft_structure(T[:, ::-1]) == 0 and dft_structure(T[None]) == 0


# -- the instrument -----------------------------------------------------------------------------------------------------------
def test_rows_are_float32_and_the_oracle_multiplies_by_the_matrix():
    for d in (8, 9, 64, 65, 74, 256):
        H = d // 2 + 1
        X, Y = D.forward_rows(d), D.inverse_rows(d)
        assert X.shape[1] == d and Y.shape[1] == 4 * H and not X.flags.writeable and not Y.flags.writeable
        assert np.array_equal(X, X.astype(np.float32).astype(np.float64)) and np.array_equal(Y, Y.astype(np.float32).astype(np.float64))
        assert not X[-1].any() and not Y[-1].any()
        imp = [r for r in X if np.count_nonzero(r) == 1 and r.max() == 1.0]
        assert len(imp) >= (d if d <= 64 else 9) and len(X) <= d + 16 and len(Y) <= 4 * H + 24
        assert np.abs(X).min(axis=1).max() > 0 and 0 < np.abs(X[-2]).min() < 2.0 ** -17          # dense rows; the 2^-20 .. 1 row
        assert np.array_equal(D.scale(d, 1, X), np.abs(X).sum(axis=1))
        junk = Y[-3]                                      # nothing but junk in the purely real bins' imaginary slots: the exact answer is 0
        assert np.count_nonzero(junk) == (4 if d % 2 == 0 else 2) and np.abs(junk @ D.matrix(d, 5).T).max() < 1e-13
        assert 0 < D.scale(d, 5, junk)[0] < 1e-4
    lengths = (8, 37, 74)
    net, cases, steps = D.transform_model(lengths, extras=(37, 74))
    assert [c.index for c in cases] == list(range(len(cases))) and D.n_transforms(cases) == 5 + 2 * 11
    model = build(net, staged=False)
    dfts = [o for o in model.ops if o["kind"] == "matvec"]
    assert len(dfts) == D.n_transforms(cases) and all(o["dft"] and o["stage"] == 1 for o in dfts)
    assert sorted(o["mode"] for o in dfts).count("set") == 4
    ref = OracleSimulator(model)
    ref.run_steps(steps)
    for c in cases:
        out = ref.probe_data(c.index)
        if c.mode == "plain":
            X = D.rows_of(c.d, c.kinds[0])
            assert np.abs(out[:len(X)] - X @ D.matrix(c.d, c.kinds[0]).T).max() < 1e-12 * max(1.0, np.abs(X).sum(axis=1).max())
            assert not out[len(X):].any()
        elif c.mode == "inc":
            X = D.rows_of(c.d, c.kinds[0])
            both = X @ D.matrix(c.d, c.kinds[0]).T + X[::-1] @ D.matrix(c.d, c.kinds[1]).T
            assert np.abs(out[:len(X)] - both).max() < 1e-11
    # the judge: the oracle against itself is exact; one element of one row moved by two bars is found, by one half is not
    want = [np.array(ref.probe_data(c.index)) for c in cases]
    res = D.judge(cases, steps, lambda c: want[c.index], lambda c: want[c.index], lambda d, k: 3.0)
    assert all(r == 0.0 for _, r, _, _ in res)
    for c in cases:
        A = D.case_scale(c, steps)
        row = int(np.argmax(A > 0))
        for f, found in ((2.0, True), (0.5, False)):
            bar = 3.0 + (D.FILTER_EXTRA if c.mode == "filter" else 0.0)
            moved = [w.copy() for w in want]
            moved[c.index][row, -1] += f * bar * D.U * A[row]
            res = D.judge(cases, steps, lambda q: moved[q.index], lambda q: want[q.index], lambda d, k: 3.0)
            assert [r > b for q, r, b, _ in res] == [found and q is c for q in cases], (c, f)
    zero = [w.copy() for w in want]
    zero[0][-1, 0] = 1e-30                                 # a row of scale 0 has to be exact
    assert D.judge(cases[:1], steps, lambda q: zero[q.index], lambda q: want[q.index], lambda d, k: 3.0)[0][1] == np.inf


def test_the_planner_restated_reaches_what_the_sweep_claims():
    D.assert_coverage()
    assert D.plan(7) is None and D.plan(6401) is None and D.plan(6399) is None          # 2 * 6399 - 1 > 6400: no convolution length
    assert D.plan(97).key() == (1, 97, 256, 1, 0, 0, (8, 8, 4)) and D.plan(97, no_inplace=True).inplace == 0
    assert D.plan(1015, 5).radices == (29, 7, 5) and D.plan(16).radices == (4, 4) and D.plan(32).radices == (8, 4)
    assert D.plan(1801).key()[2:4] == (4096, 1) and D.plan(2049).key()[2:4] == (4608, 0) and D.needs_flag(D.plan(1801))
    assert D.plan(1015, 1, four_step=True).key()[4:6] == (29, 35) or D.plan(1015, 1, four_step=True).key()[4:6] == (35, 29)
    err = "[ssn] plan item\n[ssn] dft kind 5 N 74 M 160 inplace 0 split 0x0 radices 8 5 4\n[ssn] dft kind 1 N 45 M 0 inplace 0 split 5x9 radices\nx"
    assert D.parse_listing(err) == [(5, 74, 160, 0, 0, 0, (8, 5, 4)), (1, 45, 0, 0, 5, 9, ())]
    assert D.parse_listing(err)[0] == D.plan(74, 5).key()


# -- the bars -----------------------------------------------------------------------------------------------------------------
# every radix, 2^1 and 2^4 remainders, every M of the sweep in both orders, even Bluestein lengths, dense primes of the four-step, and
# the length at which each class is worst (dft_checks.C0)
SUBSET = (8, 10, 16, 23, 29, 31, 37, 39, 45, 47, 51, 57, 64, 74, 86, 97, 106, 113, 121, 161, 225, 226, 237, 239, 255, 256)


def test_bars_come_from_the_stand_in_and_stay_below_the_worst_case():
    assert D.C == {k: 2 * v for k, v in D.C0.items()} and set(D.C) == set(D.CLASSES)
    plans = [p for fs, ni in ((False, False), (True, False), (False, True)) for p in D.sweep_plans(fs, ni)]
    for p in plans:
        assert D.C[p.cls] < D.analytic_c(p), p
    for d, big, ni, kinds in D.LONG:
        p = D.plan(d, 1, no_inplace=ni)
        assert 2 * D.C0_LONG[(d, ni)] < D.analytic_c(p) and bool(p.M) == big == D.needs_flag(p), p
    assert {r for d in SUBSET for r in D.plan(d).radices} == {2, 3, 4, 5, 7, 8, 9, 11, 13, 15, 17, 19, 23, 29, 31}
    worst = {}
    for fs, ni in ((False, False), (True, False), (False, True)):
        for p in D.sweep_plans(fs, ni, lengths=SUBSET):
            if ni and not p.M:
                continue
            r = D.standin_ratio(p)
            assert r <= D.C0[p.cls], (p, r)                # half a bar
            worst[p.cls] = max(worst.get(p.cls, 0.0), r)
    print("the stand-in's worst error / (u A) on the subset:", {k: round(v, 3) for k, v in worst.items()})
    # the subset holds the sweep's worst case of every class: the constants are not stale
    assert all(0.9 * D.C0[k] <= worst[k] for k in D.CLASSES), worst


def test_stand_in_stores():
    """``inc`` onto a non-zero destination and ``set``: what the stand-in's store does, against the matrices."""
    d = 45
    X = D.forward_rows(d)
    first = (X[::-1] @ D.matrix(d, 4).T).astype(np.float32)
    p = D.plan(d, 1)
    out = D.standin(p, X, set_mode=False, dst=first)
    A = D.scale(d, 1, X) + D.scale(d, 4, X[::-1])
    assert D.ratios(out, X @ D.matrix(d, 1).T + first.astype(np.float64), A).max() <= D.C0["direct"]
    assert np.array_equal(D.standin(p, X, set_mode=True, dst=first), D.standin(p, X))


# -- wrong devices ------------------------------------------------------------------------------------------------------------
# mutant -> (lengths, kinds, four-step engine) on which it has to fail
WRONG = {
    "twiddle-index": ((45, 121), (1, 5), False),
    "radix8-b1-b3": ((64, 40), (1, 5), False),
    "no-conj": ((45, 97), (3, 4), False),
    "slot-b": ((45, 97), (2, 4), False),
    # (only Bluestein lengths: without the chirp, junk in the Nyquist bin's imaginary slot stays in the imaginary lane, which no engine reads)
    "nyquist": ((74, 106, 226), (5,), False),
    "chirp-phase": ((97, 251), (1, 5), False),
    "fb-natural": ((97, 106), (1, 5), False),
    "unpadded": ((97, 106), (1, 5), False),
    "fourstep-twiddle": ((45, 255), (1, 5), True),
    # (the inverse kind stores all N points; the forward kinds store H of them and have no use for the last tile)
    "fourstep-tile": ((255, 248, 136), (5,), True),
    "inverse-1-over-M": ((74, 97), (5,), False),
}


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_every_wrong_device_fails_the_bar(mutant):
    assert set(WRONG) | {"inc-as-set"} == set(D.MUTANTS)
    if mutant == "inc-as-set":
        d = 45
        X = D.forward_rows(d)
        first = (X[::-1] @ D.matrix(d, 4).T).astype(np.float32)
        out = D.standin(D.plan(d, 1), X, set_mode=False, dst=first, mut=(mutant,))
        A = D.scale(d, 1, X) + D.scale(d, 4, X[::-1])
        assert D.ratios(out, X @ D.matrix(d, 1).T + first.astype(np.float64), A).max() > D.C["direct"]
        return
    lengths, kinds, four = WRONG[mutant]
    failed = []
    for d in lengths:
        for k in kinds:
            p = D.plan(d, k, four_step=four)
            r = D.standin_ratio(p, mut=(mutant,))
            assert D.standin_ratio(p) <= D.C0[p.cls]       # ... and passes unmutated
            failed.append(r > D.C[p.cls])
    assert all(failed), (mutant, failed)
