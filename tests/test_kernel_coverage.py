"""Every C-ABI entry point that launches a kernel is called directly by a GPU test file (CPU-only: reads source, loads no library).

tests/test_gpu_kernels.py and tests/test_gpu_kernel_edges.py claim to hold every such entry point against a reference.  The model tests
reach more kernels, but at sizes and tolerances that cannot see a wrong tie rule, a lost scalar tail or a grid-stride loop that never
makes a second pass; an entry point they alone reach has no direct test.  This keeps the claim true: a launching symbol of
_lib.SYMBOLS (held equal to include/dcap.h by test_abi.py) counts as reached when some tests/test_gpu_*.py file calls an ops wrapper
that reaches it (ops.<name>, or a name imported from ops) or names the symbol itself (a call through _lib.load())."""
import ast
import glob
import os
import re

# entry points that launch nothing: sizes, tile choices, kernel names, capability queries, version / error / setting getters
NON_LAUNCHING = re.compile(r"_workspace_bytes$|_tile$|_tile_config$|_kernel_name$|_supported$|_is_pointwise$|_weight_bytes$")
NON_LAUNCHING_NAMES = {"dc_version", "dc_last_error", "dc_get_persistent_cus"}

# launching symbol -> why no GPU test file reaches it directly (keep this empty: a new entry point comes with its kernel test)
ALLOWED_UNREACHED = {}


def _launching_symbols():
    from image_captioning_amd import _lib
    return sorted(s for s in _lib.SYMBOLS if s not in NON_LAUNCHING_NAMES and not NON_LAUNCHING.search(s))


def _wrappers_by_symbol(repo_root):
    """symbol -> the ops.py functions / classes that reach it: a dc_* attribute access in their body, or a call of another ops.py
    definition that reaches it (private helpers such as _conv_launch)."""
    tree = ast.parse(open(os.path.join(repo_root, "image-captioning_amd", "ops.py")).read())
    direct, calls = {}, {}
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            direct[node.name] = {n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute) and n.attr.startswith("dc_")}
            calls[node.name] = {n.id for n in ast.walk(node) if isinstance(n, ast.Name)}
    reach = {}

    def visit(name, seen):
        if name in reach:
            return reach[name]
        out = set(direct[name])
        for callee in calls[name] & set(direct):
            if callee not in seen:
                out |= visit(callee, seen | {callee})
        if len(seen) == 1:
            reach[name] = out
        return out

    by_symbol = {}
    for name in direct:
        for sym in visit(name, {name}):
            by_symbol.setdefault(sym, set()).add(name)
    return by_symbol


def _used_in_gpu_tests(repo_root):
    """(ops wrapper names called, dc_* names mentioned) over every tests/test_gpu_*.py."""
    wrappers, named = set(), set()
    for path in sorted(glob.glob(os.path.join(repo_root, "tests", "test_gpu_*.py"))):
        tree = ast.parse(open(path).read())
        aliases = {"ops"}                                             # the module fixture every kernel test file names `ops`
        for n in ast.walk(tree):
            if isinstance(n, ast.ImportFrom) and n.module in ("image_captioning_amd", "image_captioning_amd.ops"):
                for a in n.names:
                    if n.module == "image_captioning_amd" and a.name == "ops":
                        aliases.add(a.asname or a.name)
                    elif n.module == "image_captioning_amd.ops":
                        wrappers.add(a.name)
            elif isinstance(n, ast.Import):
                aliases |= {a.asname for a in n.names if a.name == "image_captioning_amd.ops" and a.asname}
        for n in ast.walk(tree):
            if isinstance(n, ast.Attribute):
                if isinstance(n.value, ast.Name) and n.value.id in aliases:
                    wrappers.add(n.attr)
                if n.attr.startswith("dc_"):
                    named.add(n.attr)
            elif isinstance(n, ast.Name) and n.id.startswith("dc_"):
                named.add(n.id)
            elif isinstance(n, ast.Constant) and isinstance(n.value, str) and re.fullmatch(r"dc_\w+", n.value):
                named.add(n.value)
    return wrappers, named


def test_the_wrapper_map_is_read_from_ops(repo_root):
    """The parse finds what is known to be there (a parser that found nothing would pass the coverage test below vacuously)."""
    by_symbol = _wrappers_by_symbol(repo_root)
    assert {"gemm"} <= by_symbol["dc_gemm_f32"]
    assert {"relu_bwd"} <= by_symbol["dc_relu_bwd_f32"] and {"relu_bwd"} <= by_symbol["dc_relu_bwd_dual_f32"]
    assert {"conv2d"} <= by_symbol["dc_conv2d_nhwc_f32"]                    # through a private launch helper
    wrappers, named = _used_in_gpu_tests(repo_root)
    assert "gemm" in wrappers and "conv2d" in wrappers
    assert len(_launching_symbols()) > 50


def test_every_launching_entry_point_has_a_direct_gpu_test(repo_root):
    by_symbol = _wrappers_by_symbol(repo_root)
    wrappers, named = _used_in_gpu_tests(repo_root)
    missing = []
    for sym in _launching_symbols():
        if sym in ALLOWED_UNREACHED or sym in named or by_symbol.get(sym, set()) & wrappers:
            continue
        via = ", ".join("ops." + w for w in sorted(by_symbol.get(sym, ()))) or "no ops wrapper"
        missing.append("%s (%s)" % (sym, via))
    assert not missing, "entry points no tests/test_gpu_*.py file calls:\n  " + "\n  ".join(missing)


def test_the_allowlist_names_only_unreached_launching_symbols(repo_root):
    by_symbol = _wrappers_by_symbol(repo_root)
    wrappers, named = _used_in_gpu_tests(repo_root)
    launching = set(_launching_symbols())
    for sym in ALLOWED_UNREACHED:
        assert sym in launching, "%s is not a launching entry point" % sym
        assert sym not in named and not by_symbol.get(sym, set()) & wrappers, "%s is reached now: drop it from ALLOWED_UNREACHED" % sym
