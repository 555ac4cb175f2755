"""Every DC_EALIGN refusal of the library has a case that provokes it (CPU-only: reads source, loads no library).

include/dcap.h promises that a pointer, leading dimension or width that breaks a 16-byte rule is refused with DC_EALIGN before anything
is launched (or served by a slower path).  tests/test_gpu_operand_placement.py provokes each refusal on the device from the REFUSALS
table of tests/_placement_cases.py; this file keeps that table complete: the message literals that follow `DC_EALIGN,` in csrc/*.hip
and *.h are exactly the literals of REFUSALS plus UNPROVOKED (literal -> written reason, kept empty).  A new DC_EALIGN site fails here
until it comes with its refusal case."""
import glob
import os
import re

import _placement_cases as P

# DC_EALIGN, "literal" ["continued literal" ...]  -- the message of a DC_REQUIRE(cond, DC_EALIGN, "...", args)
SITE = re.compile(r'DC_EALIGN\s*,\s*((?:"(?:[^"\\]|\\.)*"\s*)+)')
PIECE = re.compile(r'"((?:[^"\\]|\\.)*)"')


def _source_literals(repo_root):
    """message literal -> [file:line, ...] over the library's sources."""
    found = {}
    csrc = os.path.join(repo_root, "image-captioning_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        text = open(path).read()
        for m in SITE.finditer(text):
            literal = "".join(PIECE.findall(m.group(1)))
            found.setdefault(literal, []).append("%s:%d" % (os.path.basename(path), text.count("\n", 0, m.start()) + 1))
    return found


def test_the_parse_finds_the_sites_known_to_be_there(repo_root):
    """(a parser that found nothing would make the comparison below hold for an empty table)"""
    found = _source_literals(repo_root)
    assert "dc_gemm_f32: A/B must be 16-byte aligned with lda, ldb multiples of 4" in found           # the literal on the line after the code
    assert "dc_sumsq: x must be 16-byte aligned" in found
    assert "dc_softmax_ce: rows must be 16-byte aligned when ld %% 4 == 0" in found                   # %% kept as written
    assert "%s: X, W, bias must be 16-byte aligned" in found and len(found["%s: X, W, bias must be 16-byte aligned"]) == 2
    assert "%s: the workspace must be 16-byte aligned when N is a multiple of 4" in found            # inside a macro of dcap_internal.h
    assert len(found) >= 45


def test_every_alignment_refusal_has_a_case(repo_root):
    found = _source_literals(repo_root)
    have = P.refusal_literals()
    missing = sorted(set(found) - have - set(P.UNPROVOKED))
    assert not missing, "DC_EALIGN sites without a refusal case in tests/_placement_cases.py:\n  " + "\n  ".join(
        "%s  (%s)" % (lit, ", ".join(found[lit])) for lit in missing)
    stale = sorted((have | set(P.UNPROVOKED)) - set(found))
    assert not stale, "literals of REFUSALS / UNPROVOKED that no source file holds any more:\n  " + "\n  ".join(stale)


def test_unprovoked_entries_are_justified_and_disjoint():
    for literal, reason in P.UNPROVOKED.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4, "UNPROVOKED[%r] needs a written reason" % literal
        assert literal not in P.refusal_literals(), "%r has a case now: drop it from UNPROVOKED" % literal


def test_case_ids_are_unique_and_patterns_match_their_literals():
    ids = [case_id for _, case_id, _ in P.REFUSALS]
    assert len(ids) == len(set(ids))
    for literal in P.refusal_literals():
        assert P.literal_regex(literal).fullmatch(literal.replace("%%", "%")) or "%" in literal.replace("%%", "")
    assert P.literal_regex("%s: row set %d must be 16-byte aligned").fullmatch("dc_beam_select: row set 0 must be 16-byte aligned")
    assert P.literal_regex("a %% 4 == 0 rule").fullmatch("a % 4 == 0 rule")
    assert not P.literal_regex("dc_sumsq: x must be 16-byte aligned").fullmatch("dc_sumsq: bad arguments")


def test_the_exact_operand_builders_hold_their_precondition():
    """The host-side exactness assertions (every epilogue stage survives float32) for the shapes the GPU file uses."""
    for K in (64, 128, 136, 576, 4096):
        c = P.gemm_case(K, 70, 67, K, residual="full")
        assert c["want"].shape == (70, 67) and (c["want"] < 0).any() and (c["want"] > 0).any()
    c = P.gemm_case(1, 70, 66, 64, residual=35)
    assert c["res_rows"] == 35 and c["residual"].shape == (35, 66)
    for kh, stride, res_mode in ((1, 1, 2), (3, 1, 1), (1, 2, 0)):
        c = P.conv_case(kh, 1, 8, 8, 32, 35, kh, stride, res_mode=res_mode)
        assert c["want"].shape == (1, c["Ho"], c["Wo"], 35)
