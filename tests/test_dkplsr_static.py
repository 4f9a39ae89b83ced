"""Static checks of the direct kernel PLS surface (dkplsr, krbf, kpol): header, Python package, Julia wrapper.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_julia_wrapper import JL, _balanced, _split_top, header_protos  # noqa: E402

NEW_ENTRIES = ("jch_kernel_gram", "jch_dkplsr_fit", "jch_dkplsr_transform", "jch_dkplsr_predict")


def test_header_declares_the_entries_and_kernel_kinds():
    protos = header_protos()
    for name in NEW_ENTRIES:
        assert name in protos, name
        assert protos[name][0] == "int32_t"
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert re.search(r"#define\s+JCH_KERN_RBF\s+0\b", h)
    assert re.search(r"#define\s+JCH_KERN_POL\s+1\b", h)
    assert re.search(r"#define\s+JCH_VERSION\s+108\b", h)
    assert len(protos["jch_dkplsr_fit"][1]) == 26
    assert len(protos["jch_kernel_gram"][1]) == 17


def test_python_package_exports():
    import jchemo_hip as J
    for name in ("dkplsr", "dkplsr_", "krbf", "kpol", "Dkplsr"):
        assert hasattr(J, name), name
    for s in NEW_ENTRIES:
        assert s in J.SYMBOLS
    import dataclasses
    assert [f.name for f in dataclasses.fields(J.Dkplsr)] == ["X", "fm", "K", "kern", "xscales", "yscales", "dots"]   # src/dkplsr.jl:1-9


def test_python_kernel_keywords_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((4, 2), order="F"); Y = np.zeros((4, 1), order="F")
    with pytest.raises(ValueError):
        J.dkplsr(X, Y, nlv=1, kern="ksig")
    with pytest.raises(ValueError):
        J.dkplsr(X, Y, nlv=1, kern="krbf", degree=2)
    with pytest.raises(ValueError):
        J.dkplsr(X, Y, nlv=1, kern="kpol", sigma=2)


def _jl_function_kwargs(src, name):
    """Keyword names of every method definition `name(...; kw...)` (long or short form) in the Julia source."""
    out = []
    for m in re.finditer(r"(?:^|\n)\s*(?:function\s+)?" + re.escape(name) + r"\(", src):
        end = _balanced(src, m.end() - 1)
        sig = src[m.end():end - 1]
        if ";" not in sig:
            continue
        kw = sig.split(";", 1)[1]
        out.append([a.split("=")[0].strip() for a in _split_top(kw)])
    return out


def test_julia_module_exports_and_reference_keywords():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("dkplsr", "dkplsr!", "krbf", "kpol", "Dkplsr"):
        assert name in names, name
    # struct Dkplsr with the reference's field order (src/dkplsr.jl:1-9)
    body = re.search(r"struct Dkplsr[^\n]*\n(.*?)\nend", src, flags=re.S).group(1)
    fields = [re.match(r"\s*(\w+)", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+", ln)]
    assert fields == ["X", "fm", "K", "kern", "xscales", "yscales", "dots"]
    want = {"dkplsr": ["nlv", "kern", "scal", "ctx", "kwargs..."], "dkplsr!": ["nlv", "kern", "scal", "ctx", "kwargs..."],
            "krbf": ["gamma", "ctx"], "kpol": ["degree", "gamma", "coef0", "ctx"]}
    for name, kws in want.items():
        found = _jl_function_kwargs(src, name)
        assert found, f"no keyword method of {name}"
        assert kws in found, f"{name}: {found}"


def test_without_a_gpu_dkplsr_raises_enodev():
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: the no-device error path is not reachable")
    except ImportError:
        pass
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV
    X = np.asfortranarray(np.random.default_rng(0).random((10, 3)))
    Y = np.asfortranarray(np.random.default_rng(1).random((10, 1)))
    with pytest.raises(J.JchError) as ei:
        J.dkplsr(X, Y, nlv=2, gamma=0.5)
    assert ei.value.code == JCH_ENODEV
