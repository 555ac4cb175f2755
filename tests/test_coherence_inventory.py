"""Every place where the package derives a copy of a weight is named in tests/_coherence_cases.DERIVED_FORMS (CPU only: reads source).

Kernels read copies derived from the master weights -- Winograd and chained-pointwise packs, folded BatchNorm operands, the bf16 shadow
and per-plan casts, data-gradient packs, packed recurrent kernels -- and each copy has a refresh rule that Python enforces by hand.
tests/test_gpu_weight_coherence.py changes weights under models that hold such copies; this file keeps its table complete: it walks
the AST of every image-captioning_amd/**/*.py except ops.py (where the derivation functions are defined) and collects the call sites
of those functions.  Each (file, enclosing function, callee) must have an entry: the GPU test that covers it, or the literal reason
"rebuilt on every call" -- valid only where the call stands under no `is None` / membership test, the shape of a cache miss.  A call
site without an entry fails here until it comes with its case; so does an entry whose call site has gone."""
import ast
import os

import _coherence_cases as K

PACKAGE = "image-captioning_amd"


def _sources(repo_root):
    top = os.path.join(repo_root, PACKAGE)
    for folder, _, files in sorted(os.walk(top)):
        for name in sorted(files):
            rel = os.path.relpath(os.path.join(folder, name), top).replace(os.sep, "/")
            if name.endswith(".py") and rel != "ops.py":
                yield rel, open(os.path.join(folder, name)).read()


def _names_called(func):
    """The derivation functions a call's callee expression names: f(...), ops.f(...), (ops.f if c else ops.g)(...)."""
    found = set()
    for node in ast.walk(func):
        name = node.id if isinstance(node, ast.Name) else node.attr if isinstance(node, ast.Attribute) else None
        if name in K.DERIVED_FUNCTIONS:
            found.add(name)
    return found


def _is_cache_test(test):
    """`x is None`, `x is not None`, `k in d`, `k not in d` anywhere in a condition."""
    return any(isinstance(n, ast.Compare) and any(isinstance(op, (ast.Is, ast.IsNot, ast.In, ast.NotIn)) for op in n.ops) for n in ast.walk(test))


class _Sites(ast.NodeVisitor):
    """(enclosing function, callee, guarded) of every call of a derivation function.  guarded: the call stands inside an `if` /
    conditional expression with a cache test, or behind an `if <cache test>: ... return / continue` of an enclosing body."""

    def __init__(self):
        self.scope, self.guards, self.sites = [], [0], []

    def _scoped(self, node):
        self.scope.append(node.name)
        self.guards.append(0)
        self._body(node.body)
        self.guards.pop()
        self.scope.pop()

    visit_FunctionDef = visit_AsyncFunctionDef = _scoped

    def visit_ClassDef(self, node):
        self.scope.append(node.name)
        self.generic_visit(node)
        self.scope.pop()

    def _body(self, stmts):
        """Statements in order: an early exit under a cache test guards everything behind it in this body."""
        before = self.guards[-1]
        for st in stmts:
            self.visit(st)
            if isinstance(st, ast.If) and _is_cache_test(st.test) and any(isinstance(n, (ast.Return, ast.Continue)) for b in st.body for n in ast.walk(b)):
                self.guards[-1] += 1
        self.guards[-1] = before

    def _branching(self, node, bodies):
        self.visit(node.test)
        inc = 1 if _is_cache_test(node.test) else 0
        self.guards[-1] += inc
        for body in bodies:
            if isinstance(body, list):
                self._body(body)
            else:
                self.visit(body)
        self.guards[-1] -= inc

    def visit_If(self, node):
        self._branching(node, [node.body, node.orelse])

    def visit_IfExp(self, node):
        self._branching(node, [node.body, node.orelse])

    def visit_For(self, node):
        self.visit(node.iter)
        self._body(node.body)
        self._body(node.orelse)

    visit_While = visit_If

    def visit_With(self, node):
        for item in node.items:
            self.visit(item)
        self._body(node.body)

    def visit_Try(self, node):
        for body in (node.body, node.orelse, node.finalbody):
            self._body(body)
        for h in node.handlers:
            self._body(h.body)

    def visit_Call(self, node):
        for callee in sorted(_names_called(node.func)):
            self.sites.append((".".join(self.scope) or "<module>", callee, self.guards[-1] > 0))
        self.generic_visit(node)


def call_sites(repo_root):
    """{(file, enclosing function, callee): guarded} over the package."""
    out = {}
    for rel, text in _sources(repo_root):
        v = _Sites()
        v.visit(ast.parse(text, rel))
        for scope, callee, guarded in v.sites:
            key = (rel, scope, callee)
            out[key] = out.get(key, False) or guarded
    return out


def _weight_sites(sites):
    """Without the to_bf16 calls that cast activations or gradients (K.BF16_CASTS_OF_NON_WEIGHTS)."""
    return {k: g for k, g in sites.items() if not (k[2] == "to_bf16" and k[:2] in K.BF16_CASTS_OF_NON_WEIGHTS)}


def _gpu_tests(repo_root):
    tree = ast.parse(open(os.path.join(repo_root, "tests", K.GPU_FILE)).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def test_the_walk_finds_the_call_sites_known_to_be_there(repo_root):
    """(a walk that found nothing would make the comparisons below hold for an empty table)"""
    sites = call_sites(repo_root)
    assert sites[("encoder.py", "EncoderPlan._conv", "winograd_pack")] and sites[("encoder.py", "EncoderPlan._conv", "winograd_pack_b3")]    # one callee
    assert sites[("encoder.py", "EncoderPlan._chain", "pw_chain_pack_b3")]                     # expression, under `if n not in self._wchain`
    assert sites[("encoder.py", "EncoderPlan._conv_bf16", "to_bf16")]                          # the else of a nested if under the cache test
    assert sites[("encoder.py", "EncoderPlan._run_ops", "bn_fold")] is False                   # (`kind == "bnfold"` is no cache test)
    assert sites[("mask_rcnn_model.py", "DetectTop.folded", "bn_fold")]                        # under `if self._folded is None`
    assert sites[("text_generation_model_v2.py", "CaptionModelV2._weights_changed", "fold_bn")] is False
    assert sites[("text_generation_model_v2.py", "CaptionModelV2._decode_setup", "lstm_pack_urec")] is False
    assert sites[("text_generation_model.py", "CaptionModelV1._decode_setup", "lstm_pack_urec")] is False      # (`u % 32 == 0`: no cache test)
    assert sites[("dense_model.py", "DenseImageCapRCNN._cast_cached", "to_bf16")]              # behind `if key in cache: return`
    assert sites[("params.py", "ParamStore.refresh_shadow", "to_bf16")]
    assert not any(k[0] == "ops.py" for k in sites) and len({k[0] for k in sites}) >= 8 and len(sites) >= 24


def test_every_call_site_has_an_entry_and_every_entry_a_call_site(repo_root):
    found = set(_weight_sites(call_sites(repo_root)))
    listed = set(K.DERIVED_FORMS)
    assert not found - listed, "no entry in tests/_coherence_cases.DERIVED_FORMS for %s" % sorted(found - listed)
    assert not listed - found, "DERIVED_FORMS names call sites that no longer exist: %s" % sorted(listed - found)
    casts = {k[:2] for k in call_sites(repo_root) if k[2] == "to_bf16"}
    assert K.BF16_CASTS_OF_NON_WEIGHTS <= casts, "no to_bf16 call left in %s" % sorted(K.BF16_CASTS_OF_NON_WEIGHTS - casts)
    assert not {k[:2] for k in listed if k[2] == "to_bf16"} & K.BF16_CASTS_OF_NON_WEIGHTS


def test_every_entry_is_a_gpu_test_or_an_honest_rebuilt_on_every_call(repo_root):
    sites, tests = call_sites(repo_root), _gpu_tests(repo_root)
    assert len(tests) >= 10
    for key, entry in sorted(K.DERIVED_FORMS.items()):
        if entry == K.REBUILT:
            assert not sites.get(key, False), "%s stands under a cache test: it is not rebuilt on every call, name the GPU test that covers it" % (key,)
        else:
            assert entry in tests, "%s: tests/%s has no test %r" % (key, K.GPU_FILE, entry)
    assert sum(e == K.REBUILT for e in K.DERIVED_FORMS.values()) <= len(K.DERIVED_FORMS) // 4       # the table is about tests, not excuses


def test_the_guard_analysis_on_small_sources():
    """The three shapes of a cache miss, and a plain condition that is none."""
    src = ("def a(self):\n    if self.c is None:\n        self.c = bn_fold(1)\n    return self.c\n"
           "def b(self, k):\n    if k in self.d:\n        return self.d[k]\n    v = ops.to_bf16(self.w)\n    return v\n"
           "def c(self):\n    for n in self.names:\n        if n in self.ext:\n            continue\n        x = fold_bn(n)\n"
           "def d(self, kind):\n    if kind == 'cast':\n        ops.to_bf16(1)\n    y = (ops.winograd_pack_b3 if self.b3 else ops.winograd_pack)(2)\n"
           "class E:\n    def f(self):\n        return [lstm_pack_urec(u) if u % 32 == 0 else None for u in self.us]\n")
    v = _Sites()
    v.visit(ast.parse(src))
    assert sorted(v.sites) == [("E.f", "lstm_pack_urec", False), ("a", "bn_fold", True), ("b", "to_bf16", True), ("c", "fold_bn", True),
                               ("d", "to_bf16", False), ("d", "winograd_pack", False), ("d", "winograd_pack_b3", False)]
