"""CPU only: the host side of csrc/gemm_tn_bf16.hip answers every malformed or empty call, and every size query, as the library
did before its three routes (plain / affine / xyz, dz, grouped) were put behind one cut of the position axis and one
workspace layout each.  tests/golden/gemm_tn_host.json was RECORDED from a library built at that earlier commit by
tests/golden/make_golden_gemm_tn_host.py (which also defines the cases: every rule of every entry point broken on its own, pairs
of broken rules for the precedence of the checks, empty problems, and the slab policy and the three workspace sizes over a grid
of shapes and problem lists).  No case reaches a launch in a correct library; one that wrongly accepted a case would launch a
kernel on the never-dereferenced pointer 0x1000, so the test does not run where a GPU is visible."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN

ENTRY_POINTS = ["omnipq_gemm_tn_e16", "omnipq_gemm_tn_e16_colsum", "omnipq_gemm_tn_e16_affine", "omnipq_gemm_tn_e16_xyz_affine",
                "omnipq_gemm_tn_dz", "omnipq_gemm_tn_grouped"]
SIZE_FUNCTIONS = ["omnipq_gemm_tn_slabs", "omnipq_gemm_tn_workspace_floats", "omnipq_gemm_tn_dz_workspace_floats",
                  "omnipq_gemm_tn_grouped_workspace_floats"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_gemm_tn_host",
                                                  os.path.join(GOLDEN, "make_golden_gemm_tn_host.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gemm_tn_entry_points_answer_as_recorded(built_lib):
    if torch.cuda.is_available():
        pytest.skip("a wrongly accepted case would launch on a dummy pointer: runs on machines without a GPU only")
    gen = _generator()
    with open(os.path.join(GOLDEN, "gemm_tn_host.json")) as fh:
        table = json.load(fh)
    assert sorted({c["fn"] for c in table["calls"]}) == sorted(ENTRY_POINTS)
    assert sorted({c["fn"] for c in table["sizes"]}) == sorted(SIZE_FUNCTIONS)
    # the table is the generator's list of cases, in its order (a case added there needs a new recording)
    cases = [(fn, what, [kw.get(n, v) for n, v in gen.BASE[fn]]) for fn in gen.BASE for what, kw in gen.mutations(fn)]
    assert [(c["fn"], c["what"], c["args"]) for c in table["calls"]] == cases
    assert [(c["fn"], c["args"]) for c in table["sizes"]] == [(fn, args) for fn, args in gen.size_grid()]
    assert {c["rc"] for c in table["calls"]} == {0, gen.EINVAL}
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        assert lib.omnipq_abi_version() == table["abi_version"]
        sigs, recs = gen.signatures(lib), gen.structs(lib)
        wrong = [(c["fn"], c["what"], rc, c["rc"]) for c in table["calls"]
                 for rc in [gen.run_case(lib, sigs, recs, c["fn"], c["args"])] if rc != c["rc"]]
        assert wrong == [], (path, wrong[:10])
        wrong = [(c["fn"], c["args"], n, c["n"]) for c in table["sizes"]
                 for n in [gen.run_case(lib, sigs, recs, c["fn"], c["args"])] if n != c["n"]]
        assert wrong == [], (path, wrong[:10])
