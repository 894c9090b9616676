"""The batch plan as the host builds it (csrc/gcdm_plan.h: build_plan_host, ws_layout) against the numpy construction of tests/plan_ref.py.
No GPU and nothing loaded into Python: a stand-alone driver includes the header, is compiled with the host g++ under AddressSanitizer and
UndefinedBehaviorSanitizer, and prints every scalar and table of a PlanHost, or every entry of a WsLayout, for the case in its arguments."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import plan_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bio-diffusion_amd", "csrc")
TABLES = ("noff", "erow", "ecol", "ncnt", "rowstart", "mask", "tvalid", "mol_sub", "sub_noff", "tail_tab")
SCALARS = ("B", "N", "max_n", "K", "E", "E_real", "tail_tiles32")

DRIVER = r"""
#include "gcdm_plan.h"
#include <cstdio>
#include <cstdlib>
template <class T> static void row(const char* name, const std::vector<T>& v) {
    std::printf("%s", name);
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}
// plan D cus K B mols_per_batch[K] nn[B] has_mask mask[sum nn]   |   ws D FinG Se Ve H0 sc N E
int main(int argc, char** argv) {
    int a = 1;
    auto next = [&]() { return a < argc ? std::atoll(argv[a++]) : 0LL; };
    const std::string what = argv[a++];
    PlanDims d;
    if (what == "ws") {
        d.D = (int)next(); d.FinG = (int)next(); d.Se = (int)next(); d.Ve = (int)next(); d.H0 = (int)next(); d.sc = (int)next();
        const long long N = next(), E = next();
        const WsLayout L = ws_layout(d, N, E);
        for (const WsEntry& b : L.buf) std::printf("buf %s %zu %zu %s\n", b.id, b.floats, b.off, b.read_as ? b.read_as : "-");
        for (const WsEntry& b : L.buf)
            if (b.read_as && L.find(b.read_as) != &b) return 3;
        std::printf("total %zu\nerr %s\n", L.total, L.err.c_str());
        return 0;
    }
    d.D = (int)next(); d.cus = (int)next();
    const int K = (int)next(), B = (int)next();
    std::vector<int32_t> per, nn;
    std::vector<uint8_t> mask;
    for (int k = 0; k < K; ++k) per.push_back((int32_t)next());
    long long N = 0;
    for (int b = 0; b < B; ++b) { nn.push_back((int32_t)next()); N += nn.back() > 0 ? nn.back() : 0; }
    const bool has_mask = next() != 0;
    for (long long i = 0; has_mask && i < N; ++i) mask.push_back((uint8_t)next());
    PlanHost p;
    p.B = -7; p.noff = {42};                   // a refusal must leave these
    std::string err;
    const int rc = build_plan_host(d, B, nn.data(), has_mask ? mask.data() : nullptr, K, K ? per.data() : nullptr, p, err);
    std::printf("rc %d\nerr %s\n", rc, err.c_str());
    row("scalars", std::vector<long long>{p.B, p.N, p.max_n, p.K, (long long)p.E, (long long)p.E_real, p.tail_tiles32});
    row("noff", p.noff); row("erow", p.erow); row("ecol", p.ecol); row("ncnt", p.ncnt); row("rowstart", p.rowstart); row("mask", p.mask);
    row("tvalid", p.tvalid); row("mol_sub", p.mol_sub); row("sub_noff", p.sub_noff); row("tail_tab", p.tail_tab);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "no g++"
    tmp = tmp_path_factory.mktemp("plan_host")
    src, exe = tmp / "plan_driver.cpp", tmp / "plan_driver"
    src.write_text(DRIVER)
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        out = subprocess.run([str(exe)] + [str(int(a)) if not isinstance(a, str) else a for a in args], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])          # a sanitizer report ends the driver with a non-zero status
        return out.stdout.splitlines()
    return run


def _header_plan(driver, nn, mask=None, per_batch=None, cus=8, D=9):
    per_batch = list(per_batch or [])
    lines = driver("plan", D, cus, len(per_batch), len(nn), *per_batch, *nn, 0 if mask is None else 1, *([] if mask is None else mask))
    got = {"rc": int(lines[0].split()[1]), "err": lines[1][4:]}
    got.update(zip(SCALARS, (int(v) for v in lines[2].split()[1:])))
    for name, line in zip(TABLES, lines[3:]):
        assert line.split()[0] == name
        got[name] = np.array([int(v) for v in line.split()[1:]], dtype=np.int64)
    return got


def _assert_equal(got, ref):
    assert got["rc"] == 0, got["err"]
    for name in SCALARS:
        assert got[name] == ref[name], name
    for name in TABLES:
        assert got[name].shape == np.asarray(ref[name]).shape and (got[name] == ref[name]).all(), name


@pytest.mark.parametrize("nn", [[1], [1, 2, 3], [19, 19, 19], [181, 3, 90]], ids=str)
def test_plain_plans(driver, nn):
    got = _header_plan(driver, nn)
    _assert_equal(got, plan_ref.plan(nn))
    assert got["E"] == got["E_real"] == sum(n * n for n in nn) and got["mask"].size == 0 and got["tvalid"].size == 0 and got["mol_sub"].size == 0
    assert (got["erow"][got["rowstart"]] == np.arange(sum(nn))).all() and (got["ncnt"] == np.repeat(nn, nn)).all()


def test_masked_plans(driver):
    ends = [0, 1, 1, 0, 0, 1, 1, 1, 0]                  # sizes [4, 5], first and last atom of each molecule masked
    got = _header_plan(driver, [4, 5], mask=ends)
    _assert_equal(got, plan_ref.plan([4, 5], mask=ends))
    assert got["E"] == got["E_real"] == 2 * 2 + 3 * 3 and (got["mask"] == ends).all()
    assert (got["ncnt"] == [0, 2, 2, 0, 0, 3, 3, 3, 0]).all() and (got["rowstart"] == [0, 0, 2, 4, 4, 4, 7, 10, 13]).all()
    assert (got["erow"] == [1, 1, 2, 2, 5, 5, 5, 6, 6, 6, 7, 7, 7]).all() and (got["ecol"] == [1, 2, 1, 2, 5, 6, 7, 5, 6, 7, 5, 6, 7]).all()
    part = [1, 1, 1, 1, 0, 1, 0, 1]                     # a fully unmasked molecule beside a partly masked one
    got = _header_plan(driver, [3, 5], mask=part)
    _assert_equal(got, plan_ref.plan([3, 5], mask=part))
    assert (got["ncnt"] == [3, 3, 3, 3, 0, 3, 0, 3]).all() and (got["rowstart"] == [0, 3, 6, 9, 12, 12, 15, 15]).all() and got["E"] == 18
    # an all-true mask is no mask: exactly the unmasked plan
    got, plain = _header_plan(driver, [4, 5], mask=[1] * 9), _header_plan(driver, [4, 5])
    assert got["mask"].size == 0
    _assert_equal(got, plain)
    _assert_equal(got, plan_ref.plan([4, 5]))


def test_packed_plans(driver):
    got = _header_plan(driver, [4, 5, 3], per_batch=[2, 1])
    _assert_equal(got, plan_ref.plan([4, 5, 3], per_batch=[2, 1]))
    assert got["K"] == 2 and got["E"] == 73 and got["E_real"] == 50 and (got["tvalid"] == [41, 9]).all()
    assert (got["rowstart"][9:] == [64, 67, 70]).all()                                             # sub-batch 1 starts at slot 64
    assert (got["erow"][41:64] == got["erow"][40]).all() and (got["ecol"][41:64] == got["ecol"][40]).all()      # the padding repeats edge 40
    assert (got["mol_sub"] == [0, 0, 1]).all() and (got["sub_noff"] == [0, 9, 12]).all()
    got = _header_plan(driver, [8, 3], per_batch=[1, 1])                                           # [8] | [3]: the first sub-batch ends on the boundary
    _assert_equal(got, plan_ref.plan([8, 3], per_batch=[1, 1]))
    assert got["E"] == got["E_real"] == 73 and (got["tvalid"] == [64, 9]).all() and got["rowstart"][8] == 64
    assert (got["mol_sub"] == [0, 1]).all() and (got["sub_noff"] == [0, 8, 11]).all()
    assert got["tail_tab"].size == 0 and got["tail_tiles32"] == 0


@pytest.mark.parametrize("nn", [[4] * 40, [19] * 16, [5, 19, 7, 29, 3, 12, 19, 8, 21, 4, 17] * 3], ids=["4x40", "19x16", "ragged"])
def test_tail_table_of_a_qualifying_plan(driver, nn):
    got, ref = _header_plan(driver, nn, cus=8), plan_ref.plan(nn, cus=8)
    N = sum(nn)
    assert ref["tail_tab"].size == 64 + (N + 31) // 32, "the numpy port must qualify this case"
    _assert_equal(got, ref)
    assert got["tail_tiles32"] == (N + 31) // 32
    G = (got["E"] + 63) // 64
    assert got["tail_tab"][1:64:8].sum() == (N + 31) // 32                    # every node tile has exactly one owner
    assert got["tail_tab"][2:64:8].sum() == G + (N + 31) // 32
    waits = got["tail_tab"][64:]
    assert ((waits & 0xffff) >= 1).all() and ((waits >> 17) == 0).all()
    if nn == [19] * 16:                                                        # 5776 edges, 91 tiles: XCD boundaries cut node tiles
        assert (waits >> 16).any() and got["tail_tab"][3:64:8].any()


@pytest.mark.parametrize("nn, cus, mask, per_batch, tiles32", [
    ([40], 8, None, None, 2), ([19, 19, 19], 8, None, None, 2),               # in the size range, a node tile over more than two XCDs
    ([19], 8, None, None, 0),                                                  # 361 edges: under 64 * 8
    ([19] * 16, 7, None, None, 0),                                             # fewer than 8 workgroups
    ([19] * 16, 8, [0] + [1] * 303, None, 0),                                  # masked
    ([19] * 16, 8, None, [16], 0),                                             # packed
], ids=["40", "19x3", "19", "cus7", "masked", "packed"])
def test_plans_without_a_tail_table(driver, nn, cus, mask, per_batch, tiles32):
    got = _header_plan(driver, nn, mask=mask, per_batch=per_batch, cus=cus)
    _assert_equal(got, plan_ref.plan(nn, mask=mask, per_batch=per_batch, cus=cus))
    assert got["tail_tab"].size == 0 and got["tail_tiles32"] == tiles32


@pytest.mark.parametrize("kw, message", [
    (dict(nn=[]), "gcdm_plan_batch: bad argument"),
    (dict(nn=[3, 0, 2]), "gcdm_plan_batch: every molecule needs >= 1 atom"),
    (dict(nn=[2, 3], mask=[1, 1, 0, 0, 0]), "gcdm_plan_batch_masked: every molecule needs >= 1 unmasked atom (the reference's centroid is 0 / 0 otherwise)"),
    (dict(nn=[4096] * 128), "gcdm_plan_batch: too many edges"),
    (dict(nn=[3, 1821]), "gcdm_plan_batch: molecule too large (max_n * (3 + F) floats must fit 64 KB of LDS)"),          # 1821 x 9 floats = 65556 bytes
    (dict(nn=[3, 17], D=1000), "gcdm_plan_batch: molecule too large (max_n * (3 + F) floats must fit 64 KB of LDS)"),
    (dict(nn=[4097], D=1), "gcdm_plan_batch: molecule too large (max_n * (3 + F) floats must fit 64 KB of LDS)"),
], ids=["bad_argument", "no_atoms", "all_masked", "too_many_edges", "too_large", "too_large_wide", "over_4096_atoms"])
def test_refusals_leave_the_output_untouched(driver, kw, message):
    got = _header_plan(driver, **kw)
    assert got["rc"] == -1 and got["err"] == message
    assert got["B"] == -7 and (got["noff"] == [42]).all() and all(got[name].size == 0 for name in TABLES[1:])
    if kw.get("D") == 1000:                                                    # 16 atoms x 1000 floats is the last size that fits
        assert _header_plan(driver, [3, 16], D=1000)["rc"] == 0


def _header_ws(driver, d, n, e):
    lines = driver("ws", d["D"], d["FinG"], d["Se"], d["Ve"], d["H0"], d["sc"], n, e)
    fields = [line.split() for line in lines if line.startswith("buf ")]
    bufs = [(f[1], int(f[2]), int(f[3])) for f in fields]
    total = int(next(line for line in lines if line.startswith("total ")).split()[1])
    return bufs, total, next(line for line in lines if line.startswith("err"))[4:], {f[4]: f[1] for f in fields if f[4] != "-"}


# gcdm_debug_read's names for whole sub-buffers (the count it returns is the sub-buffer's); "agg", "chi0", "phase", "phase_node", "erow", "ecol" are not among them
READ_AS = {"x0": "X0", "x": "XC", "fbar": "FBAR", "hin": "HIN4", "h": "H4", "chi": "CHI", "pq": "PQ4", "vdi": "VDI", "vdj": "VDJ", "vel": "VEL",
           "ep": "EP4", "alpha": "AL", "u": "U", "frames": "FR"}


@pytest.mark.parametrize("case", sorted(plan_ref.DIMS))
@pytest.mark.parametrize("n, e", [(9, 41), (9, 73), (1024 * 19, 1024 * 361), (256 * 44, 256 * 44 * 44)], ids=["4+5", "packed", "1024x19", "256x44"])
def test_workspace_layout(driver, case, n, e):
    d = plan_ref.DIMS[case]
    bufs, total, err, read_as = _header_ws(driver, d, n, e)
    ref, ref_total = plan_ref.ws_offsets(d, n, e)
    assert bufs == ref and total == ref_total and err == ""
    assert all(off % 4 == 0 for _, _, off in bufs)
    assert read_as == READ_AS


@pytest.mark.parametrize("case", sorted(plan_ref.DIMS))
def test_workspace_refusal_at_4gb(driver, case):
    d = plan_ref.DIMS[case]
    b = plan_ref.first_count_over_4gb(d, 75)
    _, total, err, _ = _header_ws(driver, d, 75 * b, 5625 * b)
    assert total * 4 >= 1 << 32 and err == "gcdm_plan_batch: workspace exceeds 4 GB (buffer-addressed); split the batch"
    _, total, err, _ = _header_ws(driver, d, 75 * (b - 1), 5625 * (b - 1))
    assert total * 4 < 1 << 32 and err == ""
