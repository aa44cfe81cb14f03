"""The per-slice bound covers what it claims to cover: in the two check modules no tolerance comparison of a whole-tensor rel_l2 is left
outside kernel_checks.SLICE_SKIP, the skip and override tables name real checks with a reason each, and a check that knows (B, H, W)
hands it to every `close`."""
import ast

import branch_bwd_checks as BB
import kernel_checks as K

MODULES = (K, BB)


def _functions(mod):
    with open(mod.__file__) as f:
        tree = ast.parse(f.read())
    return {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}


def _calls(node, name):
    return [n for n in ast.walk(node) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == name]


def rel_l2_comparisons(fn):
    """the Compare nodes of a function whose left side calls rel_l2"""
    return [n for n in ast.walk(fn) if isinstance(n, ast.Compare) and _calls(n.left, "rel_l2")]


def names_in_scope(fn):
    a = fn.args
    names = {x.arg for x in a.posonlyargs + a.args + a.kwonlyargs}
    names |= {n.id for n in ast.walk(fn) if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store)}
    return names


def close_without_geom(fn):
    return [c.lineno for c in _calls(fn, "close") if len(c.args) < 4 and not any(k.arg == "geom" for k in c.keywords)]


def test_no_whole_tensor_comparison_outside_the_skip_table():
    left, converted = {}, 0
    for mod in MODULES:
        for name, fn in _functions(mod).items():
            if name in ("close", "rel_l2"):
                continue
            n = len(rel_l2_comparisons(fn))
            if n:
                left[name] = n
            converted += len(_calls(fn, "close"))
    assert left == {k: v[0] for k, v in K.SLICE_SKIP.items()}, left
    assert converted >= 85                       # the search itself still finds them


def test_tables_name_checks_that_exist_with_a_reason_each():
    fns = {}
    for mod in MODULES:
        fns.update(_functions(mod))
    for name, (count, reason) in K.SLICE_SKIP.items():
        assert name in fns and name.startswith("check_") and count > 0 and len(reason.strip()) > 40, name
    for (name, what), (factor, cause) in K.SLICE_OVERRIDES.items():
        assert name in fns and (name.startswith("check_") or name == "run_block") and _calls(fns[name], "close"), name
        assert isinstance(what, str) and what and "*" not in what
        assert K.SLICE_F < factor <= K.SLICE_F_MAX, (name, what, factor)
        assert len(cause.strip()) > 40, (name, what)


def test_checks_that_know_the_image_pass_it():
    seen = 0
    for mod in MODULES:
        for name, fn in _functions(mod).items():
            if {"B", "H", "W"} <= names_in_scope(fn) and _calls(fn, "close"):
                assert not close_without_geom(fn), "%s.%s: close without geom at line(s) %s" % (mod.__name__, name, close_without_geom(fn))
                seen += 1
    assert seen >= 18


def test_the_detectors_detect():
    bad = ast.parse("def check_x(dev, B, H, W):\n"
                    "    assert rel_l2(a, b) < TOL[dtype] and rel_l2(c, d) < 2 * tol\n"
                    "    e = rel_l2(a, b)\n"
                    "    assert torch.equal(a, b), rel_l2(a, b)\n"
                    "    close(a, b, tol, what='a')\n"
                    "    close(a, b, tol, geom=(B, H, W), what='a')\n").body[0]
    assert len(rel_l2_comparisons(bad)) == 2
    assert {"B", "H", "W"} <= names_in_scope(bad) and close_without_geom(bad) == [5]
    unpack = ast.parse("def check_y(dev, shape):\n    B, H, W = shape\n    H2 = 1\n").body[0]
    assert {"B", "H", "W"} <= names_in_scope(unpack)
