"""The coverage list of tests/test_gpu_scratch.py cannot go stale: every function include/afv_hip.h declares is either named by a row of
the cases table (tests/_scratch_cases.py) or left out there with a reason - and no entry point whose body in csrc/ mentions the staging
buffer (d_match, Blob, ensure_match_buffer) may be left out.  No GPU."""
import glob
import os
import re

import _scratch_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGING = ("d_match", "Blob", "ensure_match_buffer")


def declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "afv_hip.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(afv_[a-z0-9_]+)\s*\(", text)))


def sources():
    files = glob.glob(os.path.join(ROOT, "anyfeature-vslam_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "anyfeature-vslam_amd", "csrc", "*.h"))
    return {f: open(f).read() for f in files}


def body_of(name, src):
    """the text between the braces of the extern "C" definition of `name`, or None.  Only that text is searched: an entry point that
    reaches the staging buffer through a helper of another name is not seen here (none of the left-out ones does today)"""
    for text in src.values():
        for m in re.finditer(r'extern "C"[^;{]*?\b' + name + r"\s*\(", text):
            brace, semi = text.find("{", m.end()), text.find(";", m.end())
            if brace < 0 or 0 <= semi < brace:
                continue                                  # a declaration
            depth, k = 0, brace
            while True:
                depth += {"{": 1, "}": -1}.get(text[k], 0)
                if depth == 0:
                    return text[brace:k + 1]
                k += 1
    return None


def test_every_declared_entry_point_has_a_row_or_a_reason():
    names = declared()
    assert len(names) > 100 and "afv_frame_pose_optimize" in names and "afv_debug_paint_scratch" in names
    covered, left = SC.covered(), SC.LEFT_OUT
    assert not [n for n in names if n not in covered and n not in left], "declared, but neither in the cases table nor left out with a reason"
    assert not [n for n in left if n in covered], "both in the cases table and left out"
    assert not [n for n in list(left) + sorted(covered) if n not in names], "named here, but not declared in include/afv_hip.h"
    assert all(isinstance(r, str) and len(r) > 10 for r in left.values())


def test_nothing_that_stages_through_the_context_is_left_out():
    src = sources()
    for name in sorted(SC.LEFT_OUT):
        body = body_of(name, src)
        assert body is not None, "%s has no definition in csrc/" % name
        hit = [t for t in STAGING if t in body]
        assert not hit, "%s is left out of the cases table, but its body mentions %s" % (name, hit)
    # the search finds what it is for
    assert "d_match" in body_of("afv_frame_pose_optimize", src) and "Blob" in body_of("afv_table_fuse_points", src)


def test_the_rows_name_existing_tests():
    """a reused test function that was renamed is noticed here, not on the GPU"""
    import importlib
    import inspect
    reused = [c for c in SC.CASES if hasattr(c.make, "reused")]
    assert len(reused) > 30
    for case in reused:
        module, function, params = case.make.reused
        fn = getattr(importlib.import_module(module), function)
        sig = list(inspect.signature(fn).parameters)
        assert all(p in sig for p in params), (case.name, params, sig)
        assert all(p in params or p in ("afv", "oracle", "gpu_ctx", "fctx", "sctx", "tbl", "pairs_path", "matcher") for p in sig), (case.name, sig)
