"""The planner of the time-batched stages (csrc/ssn_stage_plan.hpp, csrc/ssn_micro_kinds.hpp) on a CPU: csrc/stage_plan_dump.cpp,
compiled once with the host compiler, prints kinds, hazards, optimised lists with their launches, zero walks and kernel choices.
Each is held to its restatement in ``stage_checks`` (``hazard``, ``optimise``, ``pack``, ``zero_walk``, ``dispatch``) on seeded
random operator lists and on hand-made ones for what the random lists do not reach."""
import itertools

import numpy as np
import pytest

import stage_checks as S
from helpers import compiled_dump

N_LISTS, N_SIG = 300, 64
A_F32_TWIN = (0.9048374180359595, 0.90483741)          # two float64s, one float32
COEFFICIENTS = A_F32_TWIN + (0.75, 0.9512294245007140)
STAGE_KINDS = (S.K_FILL, S.K_AXPY_INC, S.K_AXPY_SET, S.K_LOWPASS, S.K_TABLE, S.K_MATVEC_INC, S.K_MATVEC_SET, S.K_PROBE)
KIND_NAMES = dict(M_FILL=S.K_FILL, M_AXPY_INC=S.K_AXPY_INC, M_AXPY_SET=S.K_AXPY_SET, M_LOWPASS=S.K_LOWPASS, M_TABLE=S.K_TABLE,
                  M_MATVEC_INC=S.K_MATVEC_INC, M_MATVEC_SET=S.K_MATVEC_SET, M_PROBE=S.K_PROBE)


@pytest.fixture(scope="session")
def stage_dump(tmp_path_factory):
    return compiled_dump(tmp_path_factory, "stage_plan_dump")


# -- operator lists -------------------------------------------------------------------------------------------------------------
def op(kind, dst=0, src=0, length=1, cols=0, prev=0, a=0.0, gain=1.0):
    """An operator as ``stage_checks.batch_ops`` makes it (``gain``: what the dump narrows b from)."""
    return dict(kind=kind, dst=dst, src=src, len=length, cols=cols, prev=prev, a=a, b=(1.0 - a) * gain, gain=gain)


def tagged(ops):
    """``op``: the index in the list handed over (pieces keep it); ``table``: the ordinal of a table operator, its id."""
    tables = itertools.count()
    return [dict(o, op=i, **({"table": next(tables)} if o["kind"] == S.K_TABLE else {})) for i, o in enumerate(ops)]


def random_list(seed):
    """2 to 40 operators of the eight stage kinds on a signal vector of 64: ranges of 1 to 24 elements whose origin is one of six
    anchors with probability 0.6 (equal origins: hazard 1), ``src_prev`` on a quarter of the readers, fills of 0 among the fills."""
    rng = np.random.RandomState(seed)
    anchors = rng.randint(0, N_SIG - 1, size=6)

    def span(n=None):
        n = int(rng.randint(1, 25)) if n is None else n
        lo = int(anchors[rng.randint(0, 6)]) if rng.rand() < 0.6 else int(rng.randint(0, N_SIG))
        return min(lo, N_SIG - n), n
    out = []
    for _ in range(rng.randint(2, 41)):
        kind = STAGE_KINDS[rng.randint(0, len(STAGE_KINDS))]
        dst, n = span()
        prev = int(kind in S.READS and rng.rand() < 0.25)
        if kind in S.PRODUCTS:
            src, cols = span()
            out.append(op(kind, dst, src, n, cols, prev))
        elif kind == S.K_PROBE:
            out.append(op(kind, 0, dst, n))
        elif kind == S.K_LOWPASS:
            out.append(op(kind, dst, span(n)[0], n, 0, prev, COEFFICIENTS[rng.randint(0, 4)]))
        elif kind in (S.K_AXPY_INC, S.K_AXPY_SET):
            out.append(op(kind, dst, span(n)[0], n, 0, prev, (1.0, -1.25, 0.5)[rng.randint(0, 3)]))
        elif kind == S.K_FILL:
            out.append(op(kind, dst, 0, n, a=(0.0, 0.0, 1.5)[rng.randint(0, 3)]))
        else:
            out.append(op(kind, dst, 0, n))
    return tagged(out)


def scans(gain, between=(), prev=(0, 0)):
    return tagged([op(S.K_LOWPASS, 0, 20, 10, 0, prev[0], A_F32_TWIN[0], gain)] + list(between)
                  + [op(S.K_LOWPASS, 10, 30, 10, 0, prev[1], A_F32_TWIN[1], gain)])


def ceiling(interior):
    """A fill of 40 whose range holds ``interior`` endpoints of other operators (one-element probes of elements 0 .. interior - 1)."""
    return tagged([op(S.K_FILL, 0, 0, 40, a=0.0)] + [op(S.K_PROBE, 0, i, 1) for i in range(interior)])


def overflow(n):
    return tagged([op(S.K_FILL, i, 0, 1, a=1.5) for i in range(n)])


# b = (1 - a) gain: at gain 0 it is one value in both formats; at gain 1 the two b lie more than a float32 ulp apart (8e-9 at 0.095)
HAND_MADE = {
    "joined-scans": scans(0.0),
    "scans-apart-by-b": scans(1.0),
    "scans-apart-by-level": scans(0.0, [op(S.K_FILL, 30, 0, 10, a=1.5)]),
    "scans-apart-by-prev": scans(0.0, prev=(0, 1)),
    "ceiling-29": ceiling(29), "ceiling-30": ceiling(30), "ceiling-31": ceiling(31), "ceiling-32": ceiling(32),
    "overflow-25": overflow(25), "overflow-49": overflow(49),
}


@pytest.fixture(scope="session")
def lists():
    return [random_list(seed) for seed in range(N_LISTS)] + list(HAND_MADE.values())


def line(o):
    return "%d %d %d %d %d %d %r %r" % (o["kind"], o["dst"], o["src"], o["len"], o["cols"], o["prev"], float(o["a"]), float(o["gain"]))


def text(ops):
    return "".join(line(o) + "\n" for o in ops)


def answers(out, n):
    """The dump's answer to n lists: the lines of each, without the closing ``end``."""
    parts = out.split("end\n")
    assert len(parts) == n + 1 and parts[-1] == "", (len(parts), n)
    return [p.splitlines() for p in parts[:-1]]


def launches_of(packed):
    """``stage_checks.pack`` as (first, count) over the list it packed."""
    out, first = [], 0
    for what, item in packed:
        n = len(item) if what == "list" else 1
        out.append((first, n))
        first += n
    return out


# -- kinds --------------------------------------------------------------------------------------------------------------------
def test_kind_numbers_and_batch_flags_are_the_restated_ones(stage_dump):
    rows = {}
    for ln in stage_dump("kinds").splitlines():
        f = ln.split()
        rows[f[1]] = (int(f[0]), set(f[2:]))
    for name, number in KIND_NAMES.items():
        assert rows[name][0] == number, name
    for flag, kinds in (("ew", S.ELEMENTWISE), ("w", S.WRITES), ("r", S.READS), ("product", S.PRODUCTS)):
        assert {n for n, f in rows.values() if flag in f} == kinds, flag
    assert sorted(n for n, _ in rows.values()) == list(range(1, len(rows) + 1)) and len(rows) >= 17


# -- hazard -------------------------------------------------------------------------------------------------------------------
def test_hazard_of_every_ordered_pair(stage_dump, lists):
    pairs = [(a, b) for ops in lists for a, b in itertools.islice(itertools.combinations(ops, 2), 60)]
    got = [int(v) for v in stage_dump("hazard", stdin="".join(line(a) + "\n" + line(b) + "\n" for a, b in pairs)).split()]
    want = [S.hazard(a, b) for a, b in pairs]
    assert got == want
    assert min(want.count(c) for c in (0, 1, 2)) >= 100, [want.count(c) for c in (0, 1, 2)]


# -- plan ---------------------------------------------------------------------------------------------------------------------
def _plans(stage_dump, lists, dtype, *flags):
    out = []
    for lines in answers(stage_dump("plan", dtype, *flags, stdin="".join(text(ops) + "end\n" for ops in lists)), len(lists)):
        ops = S.parse_listing("\n".join(l for l in lines if l.startswith("[ssn]")) + "\n")
        launches = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("launch ")]
        assert len(ops) + len(launches) == len(lines)
        out.append((ops, launches))
    return out


@pytest.mark.parametrize("dtype,real", [("f32", np.float32), ("f64", np.float64)])
def test_optimised_lists_and_launches(stage_dump, lists, dtype, real):
    got = _plans(stage_dump, lists, dtype)
    unbatched = _plans(stage_dump, lists, dtype, "no-stage-batch")
    for ops, (g_ops, g_launches), (u_ops, u_launches) in zip(lists, got, unbatched):
        want = S.optimise(ops, real=real)
        assert g_ops == S.plan_key(want) and u_ops == g_ops, ops
        assert g_launches == launches_of(S.pack(want)), ops
        assert u_launches == launches_of(S.pack(want, stage_batch=False)) == [(i, 1) for i in range(len(want))], ops


def test_the_random_lists_reach_every_class():
    """Counted on the restatement alone: a later change to the generator cannot silently empty a class."""
    n = dict(cut=0, reordered=0, shared=0, clash=0, full=0)
    for seed in range(N_LISTS):
        ops = random_list(seed)
        out = S.optimise(ops)
        packed = S.pack(out)
        resets_and_sums = lambda l: sum(1 for o in l if o["kind"] in (S.K_FILL, S.K_AXPY_INC, S.K_AXPY_SET))
        n["cut"] += resets_and_sums(out) > resets_and_sums(ops)
        n["reordered"] += [o["op"] for o in out] != sorted(o["op"] for o in out)
        n["shared"] += any(what == "list" and any(S.hazard(a, b) == 1 for a, b in itertools.combinations(item, 2)) for what, item in packed)
        n["full"] += any(what == "list" and len(item) == S.MAX_BATCH_OPS for what, item in packed)
        for (what, item), (_, nxt) in zip(packed, packed[1:]):      # an element-wise launch with room left, an element-wise operator behind it
            members, head = (item if what == "list" else [item]), (nxt[0] if isinstance(nxt, list) else nxt)
            if members[0]["kind"] in S.ELEMENTWISE and len(members) < S.MAX_BATCH_OPS and head["kind"] in S.ELEMENTWISE:
                assert any(S.hazard(q, head) == 2 for q in members)
                n["clash"] += 1
                break
    assert min(n.values()) >= 20, n


def test_hand_made_lists_meet_what_they_were_made_for(stage_dump):
    """What the restatement (held to the header above) makes of the hand-made lists, and the header's own answer at the ceiling."""
    count = lambda name, real, kind: sum(1 for o in S.optimise(HAND_MADE[name], real=real) if o["kind"] == kind)
    assert count("joined-scans", np.float32, S.K_LOWPASS) == 1 and count("joined-scans", np.float64, S.K_LOWPASS) == 2
    for name in ("scans-apart-by-b", "scans-apart-by-level", "scans-apart-by-prev"):
        assert count(name, np.float32, S.K_LOWPASS) == 2 and count(name, np.float64, S.K_LOWPASS) == 2, name
    # {0, len} and the interior endpoints are the offsets: 32 of them are 31 pieces, 33 keep the fill whole
    assert [count("ceiling-%d" % k, np.float32, S.K_FILL) for k in (29, 30, 31, 32)] == [30, 31, 1, 1]
    got = _plans(stage_dump, [HAND_MADE["ceiling-%d" % k] for k in (29, 30, 31, 32)], "f32")
    assert [sum(1 for o in ops if o[0] == S.K_FILL) for ops, _ in got] == [30, 31, 1, 1]
    assert launches_of(S.pack(S.optimise(HAND_MADE["overflow-25"]))) == [(0, 24), (24, 1)]
    assert launches_of(S.pack(S.optimise(HAND_MADE["overflow-49"]))) == [(0, 24), (24, 24), (48, 1)]


# -- zero map -----------------------------------------------------------------------------------------------------------------
def _zero_walks(stage_dump, cases, dtype):
    """cases: [(operators, per block {table id: zero})] -> per case, per block {skipped index: is a set}."""
    stdin = ""
    for ops, blocks in cases:
        ids = [o["table"] for o in ops if o["kind"] == S.K_TABLE]
        stdin += text(ops) + "blocks\n" + "".join(" ".join(str(int(b[t])) for t in ids) + "\n" for b in blocks) + "end\n"
    out = []
    for (ops, blocks), lines in zip(cases, answers(stage_dump("zero", dtype, stdin=stdin), len(cases))):
        assert len(lines) == len(blocks)
        walks = []
        for n, ln in enumerate(lines):
            f = ln.split()
            assert f[:3] == ["block", str(n), "skipped"] and "set" in f
            skipped, sets = [int(v) for v in f[3:f.index("set")]], {int(v) for v in f[f.index("set") + 1:]}
            assert sets <= set(skipped)
            walks.append({i: i in sets for i in skipped})
        out.append(walks)
    return out


@pytest.mark.parametrize("dtype,real", [("f32", np.float32), ("f64", np.float64)])
def test_zero_walk_of_the_zero_model(stage_dump, dtype, real):
    """The model of the GPU module's ``zero`` case, its five blocks: the skips are the restatement's, their number the one that case
    derives from the input windows alone, the previous-row product is never among them and skipped increments mark nothing."""
    built = S.zero_model()
    model, cuts = built.model, S.cuts_of(S.ZERO_BLOCK, (S.ZERO_STEPS,))
    ops = [dict(o, gain=model.ops[o["op"]].get("gain", 1.0) if o["op"] >= 0 else 1.0) for o in S.batch_ops(model)]
    blocks, s0 = [], 0
    for B in cuts:
        blocks.append({o["table"]: not model.tables[o["table"]]["fn"].stored(range(s0 + 1, s0 + B + 1)).any() for o in ops if o["kind"] == S.K_TABLE})
        s0 += B
    assert len(blocks) == 5
    got = _zero_walks(stage_dump, [(ops, blocks)], dtype)[0]
    planned = S.optimise(ops, real=real)
    assert got == S.zero_walk(planned, blocks, True)
    assert sum(len(w) for w in got) == S.expected_skips(built.skippable, cuts) > 0
    assert any(not is_set for w in got for is_set in w.values()) and any(is_set for w in got for is_set in w.values())
    delayed = [i for i, o in enumerate(planned) if o["kind"] in S.PRODUCTS and o["prev"]]
    e_table = [o["table"] for o in planned if o["kind"] == S.K_TABLE and o["dst"] == planned[delayed[0]]["src"]]
    assert len(delayed) == 1 and len(e_table) == 1 and any(b[e_table[0]] for b in blocks) and not any(delayed[0] in w for w in got)
    assert S.zero_walk(planned, blocks, False) == [{}] * 5


@pytest.mark.parametrize("dtype,real", [("f32", np.float32), ("f64", np.float64)])
def test_zero_walk_of_the_random_lists(stage_dump, lists, dtype, real):
    rng = np.random.RandomState(1)
    cases = []
    for ops in lists:
        n_tables = sum(1 for o in ops if o["kind"] == S.K_TABLE)
        cases.append((ops, [{t: bool(rng.rand() < 0.5) for t in range(n_tables)} for _ in range(3)]))
    got = _zero_walks(stage_dump, cases, dtype)
    kinds = {True: 0, False: 0}
    prev_over_zeros = 0
    for (ops, blocks), walks in zip(cases, got):
        planned = S.optimise(ops, real=real)
        assert walks == S.zero_walk(planned, blocks, True), ops
        for w, eager in zip(walks, S.zero_walk(planned, blocks, True, skip_prev=True)):
            prev_over_zeros += len(set(eager) - set(w))
            for is_set in w.values():
                kinds[is_set] += 1
    assert kinds[True] >= 20 and kinds[False] >= 20 and prev_over_zeros >= 20, (kinds, prev_over_zeros)


# -- dispatch -----------------------------------------------------------------------------------------------------------------
def test_kernel_choice_at_every_threshold(stage_dump):
    """B 255 | 256 | 257 (chunked scan), cols 63 | 64, len 31 | 32 and B 31 | 32 (matrix cores), nothing at B = 0 or len = 0."""
    cases = list(itertools.product(STAGE_KINDS, (0, 1, 31, 32, 33), (0, 1, 63, 64, 65), (0, 1, 31, 32, 33, 255, 256, 257), (True, False)))
    got = stage_dump("dispatch", stdin="".join("%d %d %d %d %s\n" % (k, n, c, B, "f32" if f32 else "f64") for k, n, c, B, f32 in cases)).split()
    want = [S.dispatch(k, n, c, B, f32) or "nothing" for k, n, c, B, f32 in cases]
    assert got == want
    assert set(want) == {"nothing", "kb_lowpass", "kb_lowpass_chunked", "kb_gemm", "kb_gemm_mfma_f32", "kb_elementwise"}
