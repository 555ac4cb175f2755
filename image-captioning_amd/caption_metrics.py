"""Caption metrics on token ids: BLEU-1..4, ROUGE-L and CIDEr as the reference's pure-Python scorers compute them (eval/bleu,
eval/rouge, eval/cider -- the three of its five metrics that need no Java), on the host (the default) or on the device.

A sentence is a sequence of non-negative int32 ids.  Id 0 is a word like any other: padding is told by the lengths only, and what the
padded positions hold is never read.  N-gram equality is equality of the ids.

  pack_captions(cands, refs)        id lists -> CaptionBatch (padded int32 arrays + CSR indices)
  encode_strings(gens, refs)        the reference's {key: [str]} dictionaries -> id lists + the word -> id map
  score(batch, metrics, backend)    per-record and corpus values + the integer statistics
  score_predictions(gens, refs)     {'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'} of the eval_text_generation_model*.py scripts

A GROUP is the corpus of one `compute_score` call of the reference: CIDEr's document frequencies and its log N are per group (one
image in eval_densecap_image_based.py, the whole split elsewhere).  BLEU and ROUGE per record do not depend on the group; the corpus
values (BLEU_corpus, ROUGE_mean, CIDER_mean) are over ALL records of the batch.

The metrics, from their definitions (n = 4):
  BLEU (bleu_scorer.py as Bleu(4) calls it, option "closest"): guess_k = max(0, len - k + 1); correct_k = sum over the candidate's
    distinct k-grams of min(count, max over the references of count); reflen = the reference length closest to the candidate's, the
    shorter on a tie; bleu_k = (prod_{j<=k} (correct_j + 1e-15) / (guess_j + 1e-9)) ^ (1/k), times exp(1 - 1/ratio) when
    ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1.  The corpus value is the same formula on the summed statistics.
  ROUGE-L (rouge.py, beta = 1.2): F = (1 + beta^2) P R / (R + beta^2 P) with P = max over references of l / len(cand),
    R = max over references of l / len(ref); 0.0 when either is 0.  rouge="reference" (the default) takes for l what the fork's
    my_lcs returns -- its table rows alias one list, so the value is the number of positions of the SHORTER sentence (the candidate
    on equal lengths) whose token occurs anywhere in the longer one; rouge="lcs" takes the true longest common subsequence, the
    published metric.  In both an empty sentence counts as length 1 in the divisions and matches nothing (''.split(' ') is ['']);
    a record whose candidate AND one of its references are empty is outside the contract (the reference matches '' with '').
  CIDEr (cider_scorer.py, sigma = 6), per group of N records: df(g) = number of records whose reference set holds g; the weight of g
    in a sentence is tf * (log N - log max(1, df)); per order sim = sum_{g in cand} min(w_c, w_r) w_r / (|c| |r|) (no division when a
    norm is 0), times exp(-delta^2 / 2 sigma^2) with delta the difference of the two sentences' bigram counts max(len - 1, 0); the mean
    over the four orders, divided by the number of references, times 10.  A group of one record scores exactly 0.0.

backend="device" runs the per-record work in HIP (csrc/caption_metrics.hip through ops.caption_metrics / ops.caption_cider) and
returns torch tensors on the device; it takes sentences of at most MAX_DEVICE_TOKENS tokens.  Its CIDEr path numbers the n-grams with
torch.unique and therefore SYNCHRONISES with the host (unique's output size); it is an offline evaluation path, not a training-step one.
"""
import math
from collections import Counter

import numpy as np

from . import _lib

METRICS = ("BLEU", "ROUGE", "CIDER")
JAVA_METRICS = ("METEOR", "SPICE")
MAX_DEVICE_TOKENS = _lib.CAPTION_MAX_TOKENS            # include/dcap.h: one wave holds a sentence, a position per lane
N_ORDERS = 4
CIDER_SIGMA = 6.0
ROUGE_BETA = 1.2
_TINY, _SMALL = 1e-15, 1e-9
STAT_CORRECT, STAT_GUESS, STAT_TESTLEN, STAT_REFLEN, STAT_LCS_MAX, STAT_WORDS = 0, 4, 8, 9, 10, 12


class CaptionMetricsError(ValueError):
    pass


def check_metric(method):
    """The metric names score() takes; the two Java ones are refused by what they lack."""
    if method in JAVA_METRICS:
        raise CaptionMetricsError("%s needs the reference's Java jars (eval/%s: %s), which are not part of this package; "
                                  "BLEU, ROUGE and CIDER are built" % (method, method.lower(),
                                                                      "meteor-1.5.jar" if method == "METEOR" else "spice-1.0.jar"))
    if method not in METRICS:
        raise CaptionMetricsError("unknown metric %r: one of %s" % (method, ", ".join(METRICS)))
    return method


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _host(x):
    return x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)


class CaptionBatch(object):
    """cand int32 [N,Tc], cand_len int32 [N]; refs int32 [M,Tr], ref_len int32 [M]; ref_start int32 [N+1], the CSR index of a record's
    references (every record has at least one); group_start int32 [G+1], the CSR index of the groups over the records.  NumPy arrays,
    or torch tensors of one device.  The constructor refuses, by the field's name, a wrong dtype or shape, a length outside its row, a
    CSR index that does not start at 0, decreases or ends elsewhere than at the row count, a record without references and a
    negative id among the tokens the lengths cover."""

    FIELDS = ("cand", "cand_len", "refs", "ref_len", "ref_start", "group_start")

    def __init__(self, cand, cand_len, refs, ref_len, ref_start, group_start=None):
        if group_start is None:
            n = int(cand.shape[0])
            group_start = np.array([0, n] if n else [0], np.int32)
            if _is_torch(cand):
                import torch
                group_start = torch.from_numpy(group_start).to(cand.device)
        self.cand, self.cand_len, self.refs, self.ref_len, self.ref_start, self.group_start = cand, cand_len, refs, ref_len, ref_start, group_start
        self.validate()

    @property
    def N(self):
        return int(self.cand.shape[0])

    def host(self):
        """The six fields as NumPy arrays (one copy each from a device batch)."""
        return tuple(_host(getattr(self, f)) for f in self.FIELDS)

    def validate(self):
        for f in self.FIELDS:
            a = getattr(self, f)
            if not (_is_torch(a) or isinstance(a, np.ndarray)):
                raise CaptionMetricsError("CaptionBatch.%s must be a NumPy array or a torch tensor, got %s" % (f, type(a).__name__))
            if str(a.dtype).replace("torch.", "") != "int32":
                raise CaptionMetricsError("CaptionBatch.%s must be int32, got %s" % (f, a.dtype))
            if len(a.shape) != (2 if f in ("cand", "refs") else 1):
                raise CaptionMetricsError("CaptionBatch.%s must have %d dimension(s), got shape %s" % (f, 2 if f in ("cand", "refs") else 1, tuple(a.shape)))
        cand, cand_len, refs, ref_len, ref_start, group_start = self.host()
        N, M = cand.shape[0], refs.shape[0]
        for name, rows, lens, width in (("cand_len", N, cand_len, cand.shape[1]), ("ref_len", M, ref_len, refs.shape[1])):
            if lens.shape[0] != rows:
                raise CaptionMetricsError("CaptionBatch.%s must have %d entries, got %d" % (name, rows, lens.shape[0]))
            if rows and (lens.min() < 0 or lens.max() > width):
                raise CaptionMetricsError("CaptionBatch.%s: a length lies outside 0..%d, the row width" % (name, width))
        for name, idx, rows, end in (("ref_start", ref_start, N, M), ("group_start", group_start, None, N)):
            if idx.shape[0] < 1 or (rows is not None and idx.shape[0] != rows + 1):
                raise CaptionMetricsError("CaptionBatch.%s must have %s entries, got %d" % (name, "N + 1 = %d" % (rows + 1) if rows is not None else "at least one", idx.shape[0]))
            if idx[0] != 0 or idx[-1] != end or (np.diff(idx.astype(np.int64)) < 0).any():
                raise CaptionMetricsError("CaptionBatch.%s is not a CSR index: it must start at 0, never decrease and end at %d" % (name, end))
        if N and (np.diff(ref_start) < 1).any():
            raise CaptionMetricsError("CaptionBatch.ref_start: record %d has zero references; every record needs at least one"
                                      % int(np.nonzero(np.diff(ref_start) < 1)[0][0]))
        if len(group_start) > 1 and (np.diff(group_start) < 1).any():
            raise CaptionMetricsError("CaptionBatch.group_start: a group is empty")
        for name, tok, lens in (("cand", cand, cand_len), ("refs", refs, ref_len)):
            if tok.size and (tok[np.arange(tok.shape[1])[None, :] < lens[:, None]] < 0).any():
                raise CaptionMetricsError("CaptionBatch.%s holds a negative id" % name)


def _pad(sentences, name):
    lens = np.array([len(s) for s in sentences], np.int32)
    out = np.zeros((len(sentences), max(1, int(lens.max()) if len(sentences) else 1)), np.int32)
    for i, s in enumerate(sentences):
        a = np.asarray(s, dtype=np.int64).reshape(-1)
        if a.size and (a.min() < 0 or a.max() > 2 ** 31 - 1):
            raise CaptionMetricsError("pack_captions: %s %d holds an id outside 0..2^31-1" % (name, i))
        out[i, :a.size] = a
    return out, lens


def pack_captions(cands, refs, groups=None, device=None):
    """cands: N id sequences; refs: N lists of id sequences (at least one each); groups: the CSR index [G+1] of the groups over the
    records (default: one group); device: a torch device to put the arrays on (default: NumPy arrays)."""
    if len(cands) != len(refs):
        raise CaptionMetricsError("pack_captions: %d candidates but %d reference lists" % (len(cands), len(refs)))
    for i, r in enumerate(refs):
        if len(r) == 0:
            raise CaptionMetricsError("pack_captions: record %d has zero references; every record needs at least one" % i)
    cand, cand_len = _pad(list(cands), "candidate")
    flat, ref_len = _pad([s for r in refs for s in r], "reference")
    ref_start = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    group_start = None if groups is None else np.asarray(groups)
    if group_start is not None and group_start.dtype.kind in "iu":
        group_start = group_start.astype(np.int32)
    fields = [cand, cand_len, flat, ref_len, ref_start] + ([group_start] if group_start is not None else [])
    if device is not None:
        import torch
        fields = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in fields]
    return CaptionBatch(*fields)


PUNCTUATIONS = frozenset(["''", "'", "``", "`", "-LRB-", "-RRB-", "-LCB-", "-RCB-", "(", ")", "{", "}", "[", "]", '"',
                          ".", "?", "!", ",", ":", "-", "--", "...", ";"])


def default_tokenizer(text):
    """Lower-case, the Penn Treebank word rules (treebank.word_tokenize), punctuation tokens dropped.  The reference pipes the captions
    through the Java PTBTokenizer, which is not part of this package."""
    from .treebank import word_tokenize
    return [t for t in word_tokenize(text.lower()) if t not in PUNCTUATIONS]


def encode_strings(gens, refs, tokenizer=None):
    """gens {key: [str]} (one candidate each) and refs {key: [str, ...]}, the reference's dictionaries -> (keys, cand id lists, ref id
    lists, word -> id map); ids are handed out in order of first appearance."""
    tokenizer = tokenizer or default_tokenizer
    if set(gens) != set(refs):
        raise CaptionMetricsError("encode_strings: gens and refs must have the same keys")
    word_to_id = {}

    def ids(text):
        return [word_to_id.setdefault(w, len(word_to_id)) for w in tokenizer(text)]

    keys, cands, rlists = list(gens), [], []
    for k in keys:
        if len(gens[k]) != 1:
            raise CaptionMetricsError("encode_strings: gens[%r] must hold exactly one candidate" % (k,))
        cands.append(ids(gens[k][0]))
        rlists.append([ids(s) for s in refs[k]])
    return keys, cands, rlists, word_to_id


# ---------------------------------------------------------------------------------------------------------- host path

def _ngram_counts(s):
    c = Counter()
    for k in range(1, N_ORDERS + 1):
        for i in range(len(s) - k + 1):
            c[s[i:i + k]] += 1
    return c


def _quirk_lcs(a, b):
    """What the fork's my_lcs(a, b) returns: positions of the shorter sentence (b on equal lengths) whose token is in the longer."""
    if len(a) < len(b):
        a, b = b, a
    inside = set(a)
    return sum(1 for t in b if t in inside)


def _true_lcs(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        diag = 0
        for j, y in enumerate(b):
            diag, row[j + 1] = row[j + 1], (diag + 1 if x == y else max(row[j + 1], row[j]))
    return row[len(b)]


def bleu_from_stats(correct, guess, testlen, reflen):
    """[4] BLEU values of one set of statistics (a record's, or the corpus sums), in the scorer's own order of operations."""
    out, bleu = [], 1.
    for k in range(N_ORDERS):
        bleu *= (float(correct[k]) + _TINY) / (float(guess[k]) + _SMALL)
        out.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + _TINY) / (reflen + _SMALL)
    if ratio < 1:
        out = [v * math.exp(1 - 1 / ratio) for v in out]
    return out


def _rouge_value(lcs, lc, lrs):
    prec = max(l / float(max(lc, 1)) for l in lcs)
    rec = max(l / float(max(lr, 1)) for l, lr in zip(lcs, lrs))
    if prec != 0 and rec != 0:
        return ((1 + ROUGE_BETA ** 2) * prec * rec) / float(rec + ROUGE_BETA ** 2 * prec)
    return 0.0


def _score_host(batch, metrics, rouge):
    cand, cand_len, refs, ref_len, ref_start, group_start = batch.host()
    N = cand.shape[0]
    lcs_of = _quirk_lcs if rouge == "reference" else _true_lcs
    out = {"stats": np.zeros((N, STAT_WORDS), np.int32)}
    stats = out["stats"]
    C = [tuple(cand[i, :cand_len[i]].tolist()) for i in range(N)]
    R = [[tuple(refs[j, :ref_len[j]].tolist()) for j in range(ref_start[i], ref_start[i + 1])] for i in range(N)]
    want_bleu, want_rouge, want_cider = ("BLEU" in metrics), ("ROUGE" in metrics), ("CIDER" in metrics)
    cc = [_ngram_counts(c) for c in C] if (want_bleu or want_cider) else None
    rc = [[_ngram_counts(r) for r in rs] for rs in R] if (want_bleu or want_cider) else None
    if want_bleu:
        bleu = np.zeros((N_ORDERS, N))
        for i in range(N):
            best = {}
            for counts in rc[i]:
                for g, n in counts.items():
                    if n > best.get(g, 0):
                        best[g] = n
            correct = [0] * N_ORDERS
            for g, n in cc[i].items():
                correct[len(g) - 1] += min(best.get(g, 0), n)
            tl = len(C[i])
            rl = min((abs(len(r) - tl), len(r)) for r in R[i])[1]
            stats[i, STAT_CORRECT:STAT_CORRECT + 4] = correct
            stats[i, STAT_GUESS:STAT_GUESS + 4] = [max(0, tl - k + 1) for k in range(1, N_ORDERS + 1)]
            stats[i, STAT_TESTLEN], stats[i, STAT_REFLEN] = tl, rl
            bleu[:, i] = bleu_from_stats(correct, stats[i, STAT_GUESS:STAT_GUESS + 4].tolist(), tl, rl)
        out["BLEU"] = bleu
        tot = stats.astype(np.int64).sum(axis=0).tolist()
        out["BLEU_corpus"] = np.array(bleu_from_stats(tot[0:4], tot[4:8], tot[STAT_TESTLEN], tot[STAT_REFLEN])) if N else np.zeros(N_ORDERS)
    if want_rouge:
        rg = np.zeros(N)
        for i in range(N):
            lcs = [lcs_of(r, C[i]) for r in R[i]]
            stats[i, STAT_LCS_MAX] = max(lcs)
            rg[i] = _rouge_value(lcs, len(C[i]), [len(r) for r in R[i]])
        out["ROUGE"] = rg
        out["ROUGE_mean"] = float(np.mean(rg)) if N else float("nan")
    if want_cider:
        cd = np.zeros(N)
        for g0, g1 in zip(group_start[:-1], group_start[1:]):
            df = Counter()
            for i in range(g0, g1):
                df.update(set(g for counts in rc[i] for g in counts))
            log_n = np.log(float(g1 - g0))

            def vector(counts):
                vec = [dict() for _ in range(N_ORDERS)]
                for g, tf in counts.items():
                    vec[len(g) - 1][g] = float(tf) * (log_n - np.log(max(1.0, float(df.get(g, 0)))))
                return vec, [np.sqrt(sum(w * w for w in v.values())) for v in vec]

            for i in range(g0, g1):
                vc, nc = vector(cc[i])
                total = np.zeros(N_ORDERS)
                for r, counts in zip(R[i], rc[i]):
                    vr, nr = vector(counts)
                    delta = float(max(len(C[i]) - 1, 0) - max(len(r) - 1, 0))
                    for k in range(N_ORDERS):
                        val = sum(min(w, vr[k].get(g, 0.0)) * vr[k].get(g, 0.0) for g, w in vc[k].items())
                        if nc[k] != 0 and nr[k] != 0:
                            val /= nc[k] * nr[k]
                        total[k] += val * np.e ** (-(delta ** 2) / (2 * CIDER_SIGMA ** 2))
                cd[i] = np.mean(total) / len(R[i]) * 10.0
        out["CIDER"] = cd
        out["CIDER_mean"] = float(np.mean(cd)) if N else float("nan")
    return out


# -------------------------------------------------------------------------------------------------------- device path

def _check_device_lengths(batch):
    for name, lens in (("cand_len", batch.cand_len), ("ref_len", batch.ref_len)):
        if lens.shape[0] and int(lens.max()) > MAX_DEVICE_TOKENS:
            raise CaptionMetricsError("CaptionBatch.%s: a sentence of %d tokens is over the device path's limit of %d tokens; "
                                      "backend=\"host\" has no limit" % (name, int(lens.max()), MAX_DEVICE_TOKENS))


def cider_gram_tables(batch_t):
    """The CIDEr kernel's inputs from a device batch: dense n-gram ids and their document frequencies, in PyTorch plumbing.
    Returns (grams int32 [4, N + M, T], df int32 [sum of the orders' id counts], df_off [4] ints, group_n int32 [N]); grams[k - 1, s, i]
    is the id of the k-gram that starts at position i of sentence s (candidates first, then the references), -1 where none starts.
    Ids are per group (the record's group is part of the 1-gram key) and dense per order: id_k = rank of (id_{k-1} of the prefix, the
    last token) among the distinct such int64 pairs (torch.unique), so equal ids mean equal n-grams of one group and nothing is
    hashed.  df = for every id the number of distinct (record, id) pairs among the references' n-grams (unique, then bincount):
    integers, exact, and the same on every run.  Synchronises with the host for the sizes torch.unique returns."""
    import torch
    cand, cand_len, refs, ref_len, ref_start, group_start = batch_t
    dev = cand.device
    N, M = cand.shape[0], refs.shape[0]
    T = max(1, min(MAX_DEVICE_TOKENS, max(cand.shape[1], refs.shape[1])))
    tok = torch.zeros((N + M, T), dtype=torch.int64, device=dev)
    tok[:N, :min(T, cand.shape[1])] = cand[:, :T]
    tok[N:, :min(T, refs.shape[1])] = refs[:, :T]
    lens = torch.cat([cand_len, ref_len]).to(torch.int64)
    rs = ref_start.to(torch.int64)
    rec_of_ref = torch.repeat_interleave(torch.arange(N, device=dev), rs[1:] - rs[:-1])
    gs = group_start.to(torch.int64)
    sizes = gs[1:] - gs[:-1]
    group_of_rec = torch.repeat_interleave(torch.arange(sizes.shape[0], device=dev), sizes)
    rec = torch.cat([torch.arange(N, device=dev), rec_of_ref])                         # [N + M] the record of every sentence
    pos = torch.arange(T, device=dev)[None, :]
    valid = pos < lens[:, None]
    tid = torch.zeros_like(tok)
    uniq, inv = torch.unique(tok[valid], return_inverse=True)
    tid[valid] = inv
    U = max(1, int(uniq.shape[0]))
    grams = torch.full((N_ORDERS, N + M, T), -1, dtype=torch.int32, device=dev)
    prev = group_of_rec[rec][:, None].expand(N + M, T).clone()                        # the "prefix id" of a 1-gram: its group
    dfs, df_off, off = [], [], 0
    is_ref = (torch.arange(N + M, device=dev) >= N)[:, None]
    for k in range(1, N_ORDERS + 1):
        valid = pos + k <= lens[:, None]
        last = torch.roll(tid, shifts=-(k - 1), dims=1)                               # the token id at position i + k - 1
        key = prev * U + last
        uniq, inv = torch.unique(key[valid], return_inverse=True)
        G = int(uniq.shape[0])
        ids = torch.zeros_like(tok)
        ids[valid] = inv
        grams[k - 1][valid] = inv.to(torch.int32)
        in_ref = valid & is_ref
        pairs = torch.unique(rec[:, None].expand(N + M, T)[in_ref] * max(G, 1) + ids[in_ref])
        dfs.append(torch.bincount(pairs % max(G, 1), minlength=G).to(torch.int32))
        df_off.append(off)
        off += G
        prev = ids
    df = torch.cat(dfs) if off else torch.zeros((1,), dtype=torch.int32, device=dev)
    return grams, df, df_off, sizes[group_of_rec].to(torch.int32)


def _score_device(batch, metrics, rouge):
    import torch
    from . import ops
    _check_device_lengths(batch)
    t = []
    for f in CaptionBatch.FIELDS:
        a = getattr(batch, f)
        t.append(a if _is_torch(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda())
    if not t[0].is_cuda:
        raise CaptionMetricsError("score(backend=\"device\"): the batch's tensors must live on the GPU")
    cand, cand_len, refs, ref_len, ref_start, group_start = t
    N, dev = cand.shape[0], cand.device
    out = {}
    if N == 0:                                                    # empty results, no launch
        out["stats"] = torch.zeros((0, STAT_WORDS), dtype=torch.int32, device=dev)
        if "BLEU" in metrics:
            out["BLEU"], out["BLEU_corpus"] = torch.zeros((N_ORDERS, 0), dtype=torch.float64, device=dev), np.zeros(N_ORDERS)
        if "ROUGE" in metrics:
            out["ROUGE"], out["ROUGE_mean"] = torch.zeros((0,), dtype=torch.float64, device=dev), float("nan")
        if "CIDER" in metrics:
            out["CIDER"], out["CIDER_mean"] = torch.zeros((0,), dtype=torch.float64, device=dev), float("nan")
        return out
    stats, bleu, rg = ops.caption_metrics(cand, cand_len, refs, ref_len, ref_start, lcs=(rouge == "lcs"))
    out["stats"] = stats
    if "BLEU" in metrics:
        out["BLEU"] = bleu
        tot = stats.sum(dim=0, dtype=torch.int64).tolist()
        out["BLEU_corpus"] = np.array(bleu_from_stats(tot[0:4], tot[4:8], tot[STAT_TESTLEN], tot[STAT_REFLEN]))
    if "ROUGE" in metrics:
        out["ROUGE"] = rg
        out["ROUGE_mean"] = float(rg.mean().item())
    if "CIDER" in metrics:
        grams, df, df_off, group_n = cider_gram_tables(t)
        lens = torch.cat([cand_len, ref_len]).clamp(max=grams.shape[2])
        out["CIDER"] = ops.caption_cider(grams, lens, ref_start, df, df_off, group_n)
        out["CIDER_mean"] = float(out["CIDER"].mean().item())
    return out


def score(batch, metrics=METRICS, backend="host", rouge="reference"):
    """{'BLEU' [4,N], 'ROUGE' [N], 'CIDER' [N]} float64 (those asked for), the corpus values 'BLEU_corpus' [4], 'ROUGE_mean',
    'CIDER_mean', and 'stats' int32 [N,12]: correct[4], guess[4], testlen, reflen, lcs_max and one spare word (0); a metric not asked
    for leaves its statistics 0 on the host path.  backend="host": NumPy arrays.  backend="device": the per-record arrays are torch
    tensors on the batch's device (NumPy batches are copied to the current one), the corpus values host numbers; sentences of more
    than MAX_DEVICE_TOKENS tokens are refused; results are bit-identical from run to run.  A record whose candidate and one of its
    references are both empty is outside the contract of ROUGE (see the module text)."""
    if isinstance(metrics, str):
        metrics = (metrics,)
    metrics = tuple(check_metric(m) for m in metrics)
    if not isinstance(batch, CaptionBatch):
        raise CaptionMetricsError("score: batch must be a CaptionBatch (pack_captions builds one), got %s" % type(batch).__name__)
    if rouge not in ("reference", "lcs"):
        raise CaptionMetricsError("score: rouge must be \"reference\" or \"lcs\", got %r" % (rouge,))
    if backend == "host":
        return _score_host(batch, metrics, rouge)
    if backend == "device":
        return _score_device(batch, metrics, rouge)
    raise CaptionMetricsError("score: backend must be \"host\" or \"device\", got %r" % (backend,))


def score_predictions(gens, refs, backend="host", tokenizer=None):
    """What evaluate_models/eval_text_generation_model*.py: score_predictions prints, without METEOR and SPICE: the corpus values
    {'Bleu_1'..'Bleu_4', 'ROUGE_L', 'CIDEr'} of {key: [str]} dictionaries, the whole input one group."""
    _, cands, rlists, _ = encode_strings(gens, refs, tokenizer)
    res = score(pack_captions(cands, rlists), backend=backend)
    out = {"Bleu_%d" % (k + 1): float(res["BLEU_corpus"][k]) for k in range(N_ORDERS)}
    out["ROUGE_L"], out["CIDEr"] = res["ROUGE_mean"], res["CIDER_mean"]
    return out
