"""The local-model family (lwplsr, knn, lwmlr, lwplsda) is written against ONE copy of its shared plumbing: this file counts the
copies in the sources.  No GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jchemo.jl_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _all_sources():
    return {os.path.basename(p): _read(os.path.basename(p)) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))}


def _definitions(pattern):
    """(file, match) of every place under csrc/ where the pattern matches."""
    return [(name, m.group(0)) for name, src in _all_sources().items() for m in re.finditer(pattern, src)]


def _body(src, signature):
    """The text of the function whose definition starts with `signature`, braces balanced."""
    at = src.index(signature)
    i = src.index("{", at)
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        j += 1
    return src[at:j]


def test_one_ints_as_doubles_helper():
    defs = _definitions(r"size_t\s+\w*ints_as_doubles\s*\(\s*size_t")
    assert [d[0] for d in defs] == ["jch_internal.h"], defs
    assert "jch_ints_as_doubles" in defs[0][1]
    for name in ("knn.hip", "lwmlr.hip", "lwplsda.hip", "kde.hip", "gda.hip", "viperm.hip", "lwplsr_generic.hip"):
        assert "jch_ints_as_doubles(" in _read(name), name


def test_one_slab_plan_formula():
    counts = {name: _read(name).count("(160 * 1024) /") for name in ("lwmlr.hip", "lwplsda.hip", "lwplsr_dev.h")}
    assert counts == {"lwmlr.hip": 0, "lwplsda.hip": 0, "lwplsr_dev.h": 1}, counts
    assert "(160 * 1024) /" in _body(_read("lwplsr_dev.h"), "inline jch_slab_where jch_slab_plan(")
    # the two thresholds stay named constants of their files, and both kernels go through the one launcher
    assert "#define WLS_LDS_MAX (150 * 1024)" in _read("lwmlr.hip") and "#define GDA_LDS_MAX (150 * 1024)" in _read("lwplsda.hip")
    assert "jch_slab_plan(ctx, m, slab, WLS_LDS_MAX, false)" in _read("lwmlr.hip")
    assert 'jch_slab_plan(ctx, m, *slab, GDA_LDS_MAX, jch_knob("JCH_GDA_WS", 0) == 1)' in _read("lwplsda.hip")
    assert "jch_launch_slab<k_knn_wls<true>, k_knn_wls<false>>" in _read("lwmlr.hip")
    assert "jch_launch_slab<k_knn_gda<true>, k_knn_gda<false>>" in _read("lwplsda.hip")
    assert len(_definitions(r"hipFuncSetAttribute\(\(const void \*\)k_knn_(wls|gda)")) == 0
    assert len(_definitions(r"void\s+\w+_[bw]sync\s*\(\s*\)")) == 2 and "slab_bsync" in _read("lwplsr_dev.h")


def test_one_query_map_loop():
    loops = _definitions(r"for \(const auto &qm : model->qmaps\)\s*\{[^}]*jch_launch_affine_gemm[^}]*\}")
    assert [d[0] for d in loops] == ["lwplsr.hip"], loops
    assert loops[0][1] in _body(_read("lwplsr.hip"), "int32_t jch_lw_front_map(")


def test_one_label_rule():
    defs = _definitions(r"bool\s+knn_vote_better\s*\(")
    assert [d[0] for d in defs] == ["lwplsr_dev.h"], defs
    assert _definitions(r"\bbnan\b") == []                          # the hand-written chains are gone
    da = _read("lwplsda.hip")
    for kernel in ("void k_knn_gda(gda_args g)", "void k_rda_finish("):
        body = _body(da, kernel)
        assert "best < 0 || knn_vote_better(v, bv)" in body and "knn_class_counts(" in body, kernel
    assert "knn_vote_better(v, bval)" in _read("knn.hip")
    assert len(_definitions(r"void\s+knn_class_counts\s*\(")) == 1


def test_both_prepared_entries_call_the_shared_front_end():
    decl = _read("lwplsr_dev.h")
    for fn in ("jch_lw_front_check", "jch_lw_front_stage", "jch_lw_front_map"):
        assert f"int32_t {fn}(" in decl
        assert len(_definitions(r"int32_t\s+" + fn + r"\s*\([^;{]*\)\s*\{")) == 1, fn
    for name, entry in (("lwplsr.hip", 'extern "C" int32_t jch_lwplsr_predict_prepared('), ("lwplsda.hip", 'extern "C" int32_t jch_lwplsda_predict_prepared(')):
        body = _body(_read(name), entry)
        assert "JCH_TRY(jch_lw_front_check(ctx, who, model, Zq));" in body, name
        assert "jch_lw_front_stage(ctx, model, " in body and "if (!Zq) JCH_TRY(jch_lw_front_map(ctx, model, m, &qs));" in body, name
        assert body.index("jch_lw_front_check") < body.index("jch_lw_front_stage") < body.index("jch_lw_front_map"), name
        assert "jch_stage_in" not in body and "ctx->prof = jch_profile{}" not in body, name
    # the regression entry takes its first event between the staging and the query map (bench.py's cfg5 profile reads those spans)
    body = _body(_read("lwplsr.hip"), 'extern "C" int32_t jch_lwplsr_predict_prepared(')
    assert body.index("jch_lw_front_stage") < body.index("hipEvent_t ev0 = jch_ev(ctx);") < body.index("jch_lw_front_map")


def test_one_knn_args_fill_and_one_pspace_ladder():
    assert [d[0] for d in _definitions(r"a\.cri = 4\.0")] == ["lwplsr_dev.h"]
    for name in ("lwplsr.hip", "lwplsda.hip", "knn.hip"):
        assert "jch_knn_make_args(" in _read(name), name
    assert len(_definitions(r"launch_locw<16>\(ctx, g\)")) == 1
    assert "JCH_TRY(jch_launch_locw_pspace(ctx, g));" in _body(_read("lwplsr.hip"), "static int32_t lw_run(")


def test_one_fit_per_query_helper():
    src = _read("lwplsr_generic.hip")
    assert src.count("jch_plskern_fit(") == 1 and src.count("= jch_predict(") + src.count("return jch_predict(") == 1
    assert src.count("ctx->profiling = false") == 0 and src.count("lw_profiling_off quiet(ctx);") == 2 and src.count("fit.run(ctx, g, i, ") == 2
