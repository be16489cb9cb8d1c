"""The time-batched stages on the device, every operator at every step against float64 (tests/stage_checks.py is the instrument and
states the bound; tests/test_stages.py proves it on the CPU and fails every wrong device on the same case list).

Every probed element of every step has to lie within ``bound + 2 u |value|`` of the float64 evaluation, in f32 (u = 2^-24) and in
f64 (u = 2^-53, against extended precision).  Every f32 case also holds the Python restatement of ``optimise_batch`` to the library's
own listing under SSN_DEBUG_PLAN (read from stderr), from which the tests assert the kernel each operator went to and which scans
were joined.  The worst |device - float64| / bar of every case is printed before it is asserted (run with -s)."""
import numpy as np
import pytest

from sspslam_amd import simulator as PLAN
from oracle import OracleSimulator

import stage_checks as S

pytestmark = pytest.mark.gpu

VARIANTS = (("default", 0, {}), ("no stage batch", PLAN.SSN_PLAN_NO_STAGE_BATCH, {}), ("no reorder", 0, {"SSN_NO_BATCH_REORDER": "1"}))
BY_ID = {c.id: c for c in S.CASES}


@pytest.fixture(scope="module")
def Simulator():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from sspslam_amd.simulator import Simulator
    return Simulator


class Device:
    """``Simulator`` behind the three methods the instrument asks of a device; with ``capfd`` the plan listing is kept."""

    def __init__(self, Simulator, case, dtype="f32", flags=0, env=None, capfd=None):
        self.model = case.model
        if capfd is not None:
            print(capfd.readouterr().out, end="")
        with S.environment(SSN_DEBUG_PLAN="1" if capfd is not None else None, **(env or {})):
            self.sim = Simulator(None, model=self.model, dtype=dtype, block_steps=case.block, flags=flags)
        self.listing = S.parse_listing(capfd.readouterr().err) if capfd is not None else None

    def run_steps(self, n):
        self.sim.run_steps(n)

    def data(self):
        return [np.array(self.sim.data[p["probe"]]) for p in self.model.probes]

    def counters(self):
        return self.sim.counters()


def ran(Simulator, case, **kw):
    """The case on a device of its own -> (device, data); the device is closed, every operator ran time-batched."""
    dev = Device(Simulator, case, **kw)
    with dev.sim:
        S.run_case(case, dev)
        data, cnt = dev.data(), dev.counters()
        dev.tranges = {i: dev.sim.trange(sample_every=p["every"] * S.DT) for i, p in enumerate(dev.model.probes) if p["every"] != 1}
    assert cnt["launches_per_step"] == 0, cnt
    dev.data, dev.counters = (lambda: data), (lambda: cnt)
    return dev, data


@pytest.fixture(scope="module")
def products_oracle():
    ref = OracleSimulator(S.products_model().model)
    ref.run_steps(S.products_model().steps)
    return [np.array(ref.probe_data(i)) for i in range(len(ref.model.probes))]


# ---- every case, both number formats ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_f32_under_the_bound(Simulator, capfd, case):
    dev, _ = ran(Simulator, case, capfd=capfd)
    want = S.plan_key(S.optimise(S.batch_ops(case.model)))
    assert dev.listing == want, ("the restated optimise_batch differs from the listing", [x for x in zip(dev.listing, want) if x[0] != x[1]][:4],
                                 len(dev.listing), len(want))
    fails, worst = S.failures_of(case, dev)
    print("f32 %-30s worst %.3f of the bar" % (case.id, worst))
    assert not fails, fails[:6]


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.id)
def test_f64_under_the_bound_and_equal_to_the_oracle(Simulator, case, products_oracle):
    dev, data = ran(Simulator, case, dtype="f64")
    fails, worst = S.failures_of(case, dev, f32=False)
    print("f64 %-30s worst %.3f of the bar" % (case.id, worst))
    assert not fails, fails[:6]
    ev = S.evaluation(case, f32=False)
    for i, p in enumerate(case.model.probes):
        if p["every"] == 1:
            want = products_oracle[i][:case.steps] if case.family == "products" else np.asarray(ev.V[1:case.steps + 1, p["src"]:p["src"] + p["width"]], dtype=np.float64)
            np.testing.assert_allclose(data[i], want, atol=1e-12, rtol=0)


# ---- which kernel ran what ------------------------------------------------------------------------------------------------------
def test_both_gemm_kernels_at_every_threshold_and_at_ragged_tiles(Simulator, capfd):
    """From the library's listing and the restated dispatch: the product sweep meets cols >= 64, len >= 32 and B >= 32 from both sides
    with the other two conditions true, both kernels run tiles that are ragged in rows, columns and timesteps, and the products of the
    model are exactly the listed ones."""
    case = BY_ID["products-B33-83"]
    dev, _ = ran(Simulator, case, capfd=capfd)
    listed = sorted((k, l, c) for k, _, _, l, c, _ in dev.listing if k in S.PRODUCTS)
    built = sorted((S.K_MATVEC_SET if o["mode"] == "set" else S.K_MATVEC_INC, o["rows"], o["cols"]) for o in case.model.ops if o["kind"] == "matvec")
    assert listed == built and len(built) == len(S.PRODUCT_SHAPES) + 4
    got = S.reached(dev.listing, S.PRODUCT_BLOCKS)
    M, G = got["kb_gemm_mfma_f32"], got["kb_gemm"]
    for lo, hi in (((33, 63, 33), (33, 64, 33)), ((31, 65, 33), (32, 65, 33)), ((33, 64, 31), (33, 64, 32)), ((150, 100, 31), (150, 100, 32))):
        assert lo in G and hi in M, (lo, hi)
    assert any(r % 64 and c % 32 and B % 64 for r, c, B in M) and any(r % 32 and c % 32 and B % 32 for r, c, B in G)
    assert (33, 65, 33) in M and (70, 65, 100) in M          # the sliced transform (65 of 70 columns: rows padded to 68) and the product behind the hand-off
    assert set(S.reached(dev.listing, S.PRODUCT_BLOCKS, f32=False)) == {"kb_gemm", "kb_lowpass", "kb_elementwise"}


def test_scans_joined_and_kept_apart_and_both_scan_kernels(Simulator, capfd):
    case = BY_ID["scans-B64-100+1+199"]
    dev, _ = ran(Simulator, case, capfd=capfd)
    scans = [(d, n) for k, d, _, n, _, _ in dev.listing if k == S.K_LOWPASS]
    ops = [o for o in case.model.ops if o["kind"] == "lowpass"]
    coeff = lambda tau: np.exp(-S.DT / tau)
    of = lambda tau: sorted((o["dst"], o["len"]) for o in ops if abs(o["a"] - coeff(tau)) < 1e-12)
    joined = of(S.TAU_JOINED)
    assert len(joined) >= 2 and all(a[0] + a[1] == b[0] for a, b in zip(joined, joined[1:]))             # adjacent pieces in the model ...
    assert (joined[0][0], sum(n for _, n in joined)) in scans                                              # ... one scan on the device
    apart = [of(t) for t in S.TAU_APART]
    assert apart[0][-1][0] + apart[0][-1][1] == apart[1][0][0]                                             # adjacent, different coefficients
    for pieces in apart:
        assert (pieces[0][0], sum(n for _, n in pieces)) in scans
    assert not any(d <= apart[0][0][0] and d + n > apart[1][0][0] for d, n in scans)
    got = S.reached(dev.listing, S.SCAN_BLOCKS + S.CHUNKED_BLOCKS)
    assert {B for _, _, B in got["kb_lowpass"]} == set(S.SCAN_BLOCKS) and {B for _, _, B in got["kb_lowpass_chunked"]} == set(S.CHUNKED_BLOCKS)
    assert {n for n, _, _ in got["kb_lowpass_chunked"]} >= {1, 31, 32, 33, 64, 65}


# ---- element-wise launches under three plans -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in S.CASES if c.family in ("elementwise", "chain")], ids=lambda c: c.id)
def test_elementwise_plans_agree(Simulator, case):
    """Default plan, one launch per operator (SSN_PLAN_NO_STAGE_BATCH) and the builder's order (SSN_NO_BATCH_REORDER): every variant
    under the bars; f64 equal across the variants to 1e-12; how many f32 values differ is printed, not asserted (the order of a sum
    may change)."""
    f32, f64 = {}, {}
    for name, flags, env in VARIANTS:
        dev, f32[name] = ran(Simulator, case, flags=flags, env=env)
        fails, worst = S.failures_of(case, dev)
        print("f32 %-22s %-14s worst %.3f of the bar" % (case.id, name, worst))
        assert not fails, (name, fails[:6])
        dev, f64[name] = ran(Simulator, case, dtype="f64", flags=flags, env=env)
        fails, worst = S.failures_of(case, dev, f32=False)
        assert not fails, (name, fails[:6])
    for name in ("no stage batch", "no reorder"):
        for a, b in zip(f64["default"], f64[name]):
            np.testing.assert_allclose(a, b, atol=1e-12, rtol=0)
        print("f32 %-22s %-14s %d of %d values differ from the default plan's" % (
            case.id, name, sum(int((a != b).sum()) for a, b in zip(f32["default"], f32[name])), sum(a.size for a in f32["default"])))


# ---- the zero map ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_zero_skipping_changes_no_bit(Simulator, dtype):
    """The derived skip count (``failures_of``), nothing skipped under SSN_NO_ZERO_SKIP, and the two runs equal bit for bit; the
    delayed product's first row of block 2 is the product of block 1's last row although its table has no entry there."""
    case = BY_ID["zero-B64-300"]
    dev, skipping = ran(Simulator, case, dtype=dtype)
    fails, worst = S.failures_of(case, dev, f32=dtype == "f32")
    assert not fails, fails
    assert dev.counters()["batch_products_skipped"] == S.expected_skips(case.built().skippable, case.cuts) == 14
    plain, multiplied = ran(Simulator, case, dtype=dtype, env={"SSN_NO_ZERO_SKIP": "1"})
    assert plain.counters()["batch_products_skipped"] == 0
    for name, i in case.built().probes.items():
        assert np.array_equal(skipping[i], multiplied[i]), name
    d = skipping[case.built().probes["delayed"]]
    assert np.abs(d[128]).max() > 0.05 and not d[129:].any()


# ---- probes sampled inside a stage -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("case", [c for c in S.CASES if c.family == "probes"], ids=lambda c: c.id)
def test_sampled_probes(Simulator, case, dtype):
    """``sample_every`` of 3 and 7 timesteps against blocks of 64 and 256, runs cut into uneven calls: counts and times equal
    ``trange(sample_every=)``, every sample is the unsampled probe's row."""
    dev, data = ran(Simulator, case, dtype=dtype)
    assert sorted(p["every"] for p in case.model.probes) == [1, 1, 3, 3, 7, 7]
    fails = S.sampling_failures(case, data, dev.tranges)
    assert not fails, fails
