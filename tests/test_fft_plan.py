"""The FFT planner (csrc/ssn_fft_plan.hpp) on a CPU: csrc/fft_plan_dump.cpp, compiled once with the host compiler, prints the routes
and tables that k_dft and the binder are planned with.  Routes are held to the two independent restatements in Python
(``dft_checks.plan``, ``bind_checks.plan``), tables to float64 NumPy."""
import numpy as np
import pytest

import bind_checks as B
import dft_checks as D
from helpers import compiled_dump

ROUTES = ("stockham-inplace", "stockham-outofplace", "fourstep-real", "fourstep-complex")
LENGTHS = sorted(set(range(2, 513)) | {e[0] for e in D.LONG} | set(B.LENGTHS) | {3199, 3200, 3201, 6400, 6401})
CHIRP_LENGTHS = (74, 97, 151, 239, 1801, 3199)
ULP = 2.0 ** -23          # both sides round a double that is right to well under a float32 ulp: one ulp of a value <= 1 apart at most


@pytest.fixture(scope="session")
def dump(tmp_path_factory):
    return compiled_dump(tmp_path_factory, "fft_plan_dump")


def _parse_route(line):
    f = line.split()
    assert f[1::2][:8] == ["d", "L", "M", "inplace", "split", "threads", "lds", "radices"], line
    n1, n2 = f[10].split("x")
    return f[0], int(f[2]), dict(L=int(f[4]), M=int(f[6]), inplace=int(f[8]), N1=int(n1), N2=int(n2), threads=int(f[12]), lds=int(f[14]),
                                 radices=tuple(int(v) for v in f[16:]))


@pytest.fixture(scope="session")
def routes(dump):
    out = {}
    for line in dump("routes", *LENGTHS).splitlines():
        name, d, r = _parse_route(line)
        out[name, d] = r
    assert len(out) == len(ROUTES) * len(LENGTHS)
    return out


@pytest.fixture(scope="session")
def tables(dump):
    cache = {}

    def get(name, d):
        if (name, d) not in cache:
            lines = dump("tables", name, d).splitlines()
            t = {"route": _parse_route(lines[0])[2]}
            for line in lines[1:]:
                key, hexed = line.split()
                a = np.frombuffer(bytes.fromhex(hexed), dtype=np.float32)
                t[key] = a if key in ("g1", "g2") else a.reshape(-1, 2)
            cache[name, d] = t
        return cache[name, d]
    return get


def _same(route, plan):
    """A route of the dump against a ``dft_checks.Plan`` (None: no route)."""
    if plan is None:
        return route["L"] == 0
    return (route["L"], route["M"], route["inplace"], route["N1"], route["N2"], route["radices"]) == \
        (plan.M or plan.N, plan.M, plan.inplace, plan.N1, plan.N2, plan.radices)


# -- routes -------------------------------------------------------------------------------------------------------------------
def test_stockham_routes_are_the_python_planner_s(routes):
    """Every swept length from 8 (the bound of ``plan_dft``, which stays with the caller), in place allowed and forbidden."""
    for d in LENGTHS:
        if d < 8:
            continue
        for kind in (1, 5):
            assert _same(routes["stockham-inplace", d], D.plan(d, kind, False, False)), (d, routes["stockham-inplace", d])
            assert _same(routes["stockham-outofplace", d], D.plan(d, kind, False, True)), (d, routes["stockham-outofplace", d])
    assert routes["stockham-inplace", 3199]["M"] == 6400 and routes["stockham-inplace", 3200]["M"] == 0
    assert routes["stockham-inplace", 3201]["L"] == 0 and routes["stockham-inplace", 6400]["L"] == 6400 and routes["stockham-inplace", 6401]["L"] == 0


def test_the_binder_s_route_is_the_stockham_route_out_of_place(routes):
    """Also for d in 2..7, where ``plan_dft`` has no route; the workgroup and the LDS bytes are the ones ``bind_checks`` restates."""
    for d in LENGTHS:
        r, want = routes["stockham-outofplace", d], B.plan(d)
        if want is None:
            assert r["L"] == 0, (d, r)
            continue
        assert (r["L"], r["M"], r["inplace"], r["N1"], r["N2"], r["radices"]) == (want.L, want.M, 0, 0, 0, want.radices), (d, r)
        assert r["threads"] == want.threads and r["lds"] == 24 * want.L, (d, r)
    assert all(B.plan(d) is not None for d in range(2, 8))


def test_in_place_changes_the_engine_and_nothing_else(routes):
    n_inplace = 0
    for d in LENGTHS:
        a, b = routes["stockham-inplace", d], routes["stockham-outofplace", d]
        assert {k: v for k, v in a.items() if k not in ("inplace", "threads", "lds")} == \
            {k: v for k, v in b.items() if k not in ("inplace", "threads", "lds")}, d
        if a["inplace"]:
            n_inplace += 1
            M, rmin = a["M"], min(a["radices"])
            assert M > 0 and set(a["radices"]) <= {2, 4, 8}
            assert a["threads"] == min(1024, max(64, (M // 8 + 63) // 64 * 64)) and a["lds"] == 8 * (M + M // 8 + M // rmin), (d, a)
        else:
            assert a == b, d
    assert n_inplace >= 60


def test_four_step_routes_are_the_python_planner_s(routes):
    """``dft_checks.plan`` falls back to the Stockham passes where the four-step engine has no route: the chooser says "no route" there."""
    seen = set()
    for d in LENGTHS:
        if d < 8:
            continue
        for name, kind in (("fourstep-real", 1), ("fourstep-complex", 5)):
            r, want = routes[name, d], D.plan(d, kind, True, False)
            if want is None or not want.N1:
                assert r["L"] == 0, (d, name, r)
                continue
            assert _same(r, want), (d, name, r)
            tasks = ((r["N1"] + 15) // 16) * ((r["N2"] + 15) // 16)
            assert r["threads"] == min(1024, max(256, 64 * tasks)) and r["lds"] == 16 * r["L"], (d, name, r)
            seen.add(want.cls)
    assert seen == {"fourstep", "fourstep-bluestein"}


# -- tables -------------------------------------------------------------------------------------------------------------------
def _chirp64(d):
    n = np.arange(d, dtype=np.int64)
    return np.exp(-1j * np.pi * ((n * n) % (2 * d)) / d)


def test_twiddles_and_chirp_against_float64(tables):
    for d in CHIRP_LENGTHS + (2, 55, 1015):
        t = tables("stockham-outofplace", d)
        L = t["route"]["L"]
        tw = np.exp(-2j * np.pi * np.arange(L) / L)
        assert t["twiddles"].shape == (L, 2)
        assert np.abs(t["twiddles"][:, 0] - tw.real).max() <= ULP and np.abs(t["twiddles"][:, 1] - tw.imag).max() <= ULP, d
        if d in CHIRP_LENGTHS:
            w = _chirp64(d)
            assert t["route"]["M"] >= 2 * d - 1 and t["chirp"].shape == (d, 2)
            assert np.abs(t["chirp"][:, 0] - w.real).max() <= ULP and np.abs(t["chirp"][:, 1] - w.imag).max() <= ULP, d
        else:
            assert t["route"]["M"] == 0 and "chirp" not in t and "spectrum" not in t


def test_chirp_spectrum_against_numpy_fft(tables):
    """|fb_k| <= (2d - 1) / M <= 1, and the float64 transform's own error is orders of magnitude below a float32 ulp."""
    for d in CHIRP_LENGTHS:
        t = tables("stockham-outofplace", d)
        M = t["route"]["M"]
        w = _chirp64(d)
        b = np.zeros(M, complex)
        b[:d] = w.conj()
        b[M - np.arange(1, d)] = w[1:].conj()
        fb = np.fft.fft(b) / M
        assert t["spectrum"].shape == (M, 2)
        assert np.abs(t["spectrum"][:, 0] - fb.real).max() <= ULP and np.abs(t["spectrum"][:, 1] - fb.imag).max() <= ULP, (d, M)
    assert tables("stockham-outofplace", 74)["route"]["M"] == 160 and tables("stockham-outofplace", 3199)["route"]["M"] == 6400


def test_in_place_spectrum_is_the_other_one_moved(tables):
    """Bit for bit: entry k of the out-of-place table lies at ``dif_position(k)`` of the in-place one."""
    n = 0
    for d in CHIRP_LENGTHS:
        a, b = tables("stockham-inplace", d), tables("stockham-outofplace", d)
        assert np.array_equal(a["twiddles"].view(np.uint32), b["twiddles"].view(np.uint32))
        assert np.array_equal(a["chirp"].view(np.uint32), b["chirp"].view(np.uint32))
        if not a["route"]["inplace"]:
            assert np.array_equal(a["spectrum"].view(np.uint32), b["spectrum"].view(np.uint32)), d
            continue
        n += 1
        M = a["route"]["M"]
        pos = D.dif_position(np.arange(M), M, a["route"]["radices"])
        assert sorted(pos) == list(range(M)) and not np.array_equal(pos, np.arange(M))
        assert np.array_equal(a["spectrum"].view(np.uint32)[pos], b["spectrum"].view(np.uint32)), d
    assert n >= 2          # (97 -> 256, 1801 -> 4096)


def _dft4_matrix64(N):
    """The closed form of the comment in ssn_fft_plan.hpp: [tile pair p][re | im outputs][k step][lane], float64."""
    P, Np = (N + 15) // 16, (N + 3) // 4 * 4
    KS = 2 * Np // 4
    p, part, ks, l = np.meshgrid(np.arange(P), np.arange(2), np.arange(KS), np.arange(64), indexing="ij")
    k1, k = 16 * p + (l & 15), 4 * ks + (l >> 4)
    real_in = k < Np
    n = np.where(real_in, k, k - Np)
    th = 2.0 * np.pi * ((k1 * n) % N) / N
    v = np.where(part == 0, np.where(real_in, np.cos(th), np.sin(th)), np.where(real_in, -np.sin(th), np.cos(th)))
    return np.where((k1 < N) & (n < N), v, 0.0).reshape(-1), ((k1 < N) & (n < N)).reshape(-1)


def test_four_step_matrices_against_the_closed_form(tables):
    """A prime length (one dense DFT: 97 x 1 for real input, 1 x 97 for complex) and a composite one."""
    splits = set()
    for name, d in (("fourstep-real", 97), ("fourstep-complex", 97), ("fourstep-real", 240), ("fourstep-complex", 240)):
        t = tables(name, d)
        r = t["route"]
        assert r["N1"] * r["N2"] == d and r["M"] == 0
        splits.add((r["N1"], r["N2"]))
        for key, N in (("g1", r["N1"]), ("g2", r["N2"])):
            want, inside = _dft4_matrix64(N)
            assert t[key].shape == want.shape, (name, d, key)
            assert np.abs(t[key] - want).max() <= ULP and not np.any(t[key][~inside]), (name, d, key)
    assert {(97, 1), (1, 97)} <= splits and any(a > 1 and b > 1 for a, b in splits)
