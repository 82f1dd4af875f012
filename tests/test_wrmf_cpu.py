"""WRMF without a GPU: the C ABI's surface and layout (include/wrmf.h), and the fixtures
(tests/golden/wrmf_cases.npz, written by make_golden_wrmf.py from the reference's own fit())
against the numpy restatement (tests/wrmf_numpy.py) in both Gram modes."""
import ctypes
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import wrmf_numpy as W
from conftest import GOLDEN, ROOT

ALPHA, LAMBDA, SEED = 40, 0.1, 2019


def load_cases():
    z = np.load(os.path.join(GOLDEN, "wrmf_cases.npz"))
    out = {}
    for name in z["cases"]:
        name = str(name)
        U, I, d, epochs = (int(v) for v in z[f"{name}_shape"])
        out[name] = dict(U=U, I=I, d=d, epochs=epochs,
                         csr=(z[f"{name}_indptr"], z[f"{name}_indices"], z[f"{name}_data"], (U, I)),
                         **{k: z[f"{name}_{k}"] for k in ("X0", "Y0", "X", "Y")},
                         dist_X=float(z[f"{name}_dist_X"]), dist_Y=float(z[f"{name}_dist_Y"]))
    return out


CASES = load_cases()


def conf_of(c):
    indptr, indices, data, shape = c["csr"]
    return indptr, indices, ALPHA * data, shape


@pytest.fixture(scope="module")
def restated():
    """The restatement's (X, Y) per case and mode, computed once."""
    return {(n, g): W.fit(conf_of(c), c["X0"], c["Y0"], LAMBDA, c["epochs"], gram=g)
            for n, c in CASES.items() for g in ("reference", "fresh")}


def header_functions():
    with open(os.path.join(ROOT, "include", "wrmf.h")) as f:
        return sorted(set(re.findall(r"^int (wrmf_\w+)\(", f.read(), re.M)))


def test_library_exports_every_symbol_of_the_header(rl):
    names = header_functions()
    assert len(names) == 9, names
    L = ctypes.CDLL(rl.LIB_PATH)
    assert set(names) == set(rl._lib.WRMF_SIGNATURES)
    for n in names:
        assert hasattr(L, n), n
        assert n in rl._lib.WRMF_SIGNATURES, n


def test_config_offsets_match_the_c_header(rl, tmp_path):
    """Every wrmf_config / wrmf_stats field at the offset a C compiler gives it."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    wr = import_module("recommend-lib_amd.wrmf")
    cfg = [f for f, _ in wr.WrmfConfig._fields_]
    st = [f for f, _ in wr.WrmfStats._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "wrmf.h"', "int main(void) {",
             '  printf("config %zu\\n", sizeof(wrmf_config));', '  printf("stats %zu\\n", sizeof(wrmf_stats));']
    lines += [f'  printf("c.{f} %zu\\n", offsetof(wrmf_config, {f}));' for f in cfg]
    lines += [f'  printf("s.{f} %zu\\n", offsetof(wrmf_stats, {f}));' for f in st]
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                 text=True).stdout.splitlines())
    assert int(got["config"]) == ctypes.sizeof(wr.WrmfConfig)
    assert int(got["stats"]) == ctypes.sizeof(wr.WrmfStats)
    for f in cfg:
        assert int(got[f"c.{f}"]) == getattr(wr.WrmfConfig, f).offset, f
    for f in st:
        assert int(got[f"s.{f}"]) == getattr(wr.WrmfStats, f).offset, f


@pytest.mark.parametrize("name", list(CASES))
def test_fixture_has_its_edge_rows(name):
    c = CASES[name]
    indptr, indices, data, (U, I) = c["csr"]
    nnz = np.diff(indptr)
    assert nnz[3] == 0 and 5 not in indices
    assert nnz[7] == (I + 1) // 2 and (indices[indptr[7]:indptr[8]] % 2 == 0).all()
    assert nnz[9] == 1 and indices[indptr[9]] == 11
    assert set(np.unique(data)) <= {1.0, 2.0, 3.0, 4.0, 5.0}
    assert (c["X"][3] == 0).all() and (c["Y"][5] == 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_in_reference_mode_is_within_the_stored_distance(name, restated):
    """Pins the fixture: the stored dist_* are what the restatement gives."""
    c = CASES[name]
    Xn, Yn = restated[name, "reference"]
    for ref, got, dist in ((c["X"], Xn, c["dist_X"]), (c["Y"], Yn, c["dist_Y"])):
        assert 0 < dist < 1e-6
        assert np.abs(ref - got).max() / np.abs(ref).max() <= dist


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_in_fresh_mode_is_far_from_the_goldens(name, restated):
    c = CASES[name]
    Xn, Yn = restated[name, "fresh"]
    assert np.abs(c["X"] - Xn).max() > 1.0


@pytest.mark.parametrize("name", list(CASES))
def test_initial_factors_equal_the_references_bitwise(rl, name):
    """The draw the constructor makes (WRMF.initial_factors): users first, then items."""
    c = CASES[name]
    _, X0, Y0 = rl.WRMF.initial_factors(c["U"], c["I"], c["d"], SEED)
    assert X0.dtype == np.float64 and np.array_equal(X0, c["X0"]) and np.array_equal(Y0, c["Y0"])
