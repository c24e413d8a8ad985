"""The fast scan's upload-time decode descriptors as plain host C++:
tools/verify_fast_desc.cpp builds one store per vector encoding through the C
API, plus random vectors and the bench law, and checks fast_desc.h's
descriptor field for field against a restatement of the device's vector
open, then replays the kernel's four-rows-per-lane decode lane by lane: every
row bit for bit against the element readers, nothing written past the last
4-row group, and at most 6 bytes loaded past a vector's end. No GPU, nothing
loaded into Python (hipcc only supplies the include path of the store's source
file)."""
import re

import pytest

from verifier_run import STORE_SRC, run_verifier

STORES = ["tconst", "t8u", "t16s", "t16u", "t32", "t8s", "traw",
          "v2u", "v4u", "v8s", "v8u", "v16s", "v16u", "v32", "vconst", "vneg",
          "vbig", "vsteep", "vraw", "vresets", "random", "bench"]
FIELDS = ("series", "fields", "rows", "exact32", "resid", "overread", "mismatches")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return run_verifier("verify_fast_desc", tmp_path_factory.mktemp("fd"),
                        flags=["-fopenmp"], sources=[STORE_SRC], key="store")


def test_descriptors_and_decode_match_element_readers(report):
    rc, _, rows = report
    assert sorted(rows) == sorted(STORES)
    for name, r in rows.items():
        assert tuple(r) == FIELDS, name
        assert r["mismatches"] == 0, name
        assert r["overread"] <= 6, name
    assert rc == 0


def test_bench_law_values_take_the_exact32_path(report):
    _, out, _ = report
    assert re.search(r"^bench-law series with val_exact32: 20000 of 20000$", out, re.M)
