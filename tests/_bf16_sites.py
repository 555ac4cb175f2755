"""Which matrix products of a joint-model train step run from bf16 copies of their operands, for the parity tests that hold the bf16 step
to a float64 oracle that rounds where the device rounds (oracle/np_models.py, the `quant` hook).  A plain module, no fixtures; NumPy only
at import (the package is imported inside the functions: its predicates, not copies of them, decide wherever they are callable).

  planned_sites(dims)   every product site of the step -> Site(kind, bf16, shape): what the model's own routing gives for these sizes,
                        with no launch (ops.wgrad_bf16_supported / ops.conv_bf16_supported / ops.vocab_ce_supported; the three inline
                        predicates -- RoiHead._mm's use_b, EncoderPlan._conv's bf16-storage test and CaptionModelV1's du_b / emb_b --
                        are restated here, and SiteRecorder is what keeps the restatement honest);
  Bf16Policy            the `quant` of a set of sites: O.to_bf16 there, identity elsewhere; it records which operands it rounded and
                        refuses a site it does not know;
  SiteRecorder          tests/_op_recorder.Recorder + the shapes of every top-level bf16-pipe launch and every fp32 gemm / conv launch
                        of one forward_backward, plus the plan's forward convolutions (they are launched through the plan, captured);
  check_sites           launches on the bf16 pipe == products the policy rounded, per kind; both lists are printed when they differ;
  compare / assert_close  per-tensor relative L2 error against a tolerance per tensor group, the eight worst tensors on failure.

What the hand-over does to the comparison's reach (Bf16Policy): the oracle multiplies the device's own operand copies, so an error
UPSTREAM of a handed-over operand is seen by that operand's check, not by the gradient tolerances: at REACH = 2^-13 of the operand's
largest entry, elementwise -- entries much smaller than the largest may sit far from their own rounding and pass -- plus the fp32
reductions (biases, BatchNorm parameters) that read the unrounded values.  The 1e-7-grade tolerances hold each PRODUCT given its operands
and everything that is not a product operand; the planted errors of tests/test_bf16_sites.py show both kinds being caught.

Site names are those of the oracle's hook: '<layer>:fwd|dgrad|wgrad', the decoder's split layers 'imgcap_lstm1.emb' / '.feat' / '.rec',
'imgcap_lstm2.rec', 'imgcap_lstm_d1.h' / '.feat', the RPN layers per map 'rpn_conv_shared@P2'.  The device fuses rpn_class_raw and
rpn_bbox_pred into one launch (rpn_head): the two oracle products of a map count as one (FUSED)."""
import collections

import numpy as np

from oracle import np_oracle as O

from _op_recorder import Recorder

Site = collections.namedtuple("Site", "kind bf16 shape")          # kind: 'gemm' | 'conv' | 'wgrad' | 'vocab'; shape: what a launch record shows
Dims = collections.namedtuple("Dims", "S V T R E units blocks backbone_from compute_dtype conv_bf16")
FUSED = {"rpn_class_raw": "rpn_head", "rpn_bbox_pred": "rpn_head"}
GROUPS = ("decoder", "head", "fpn_rpn", "trunk")
FEAT, D1, POOL, FPN_C = 1024, 1024, 7, 256


def dims(S, V, T, R, blocks, backbone_from=None, compute_dtype="bf16", conv_bf16=False, E=300, units=512):
    """R: RoI rows of the step (TRAIN_ROIS_PER_IMAGE x IMAGES_PER_GPU); conv_bf16: conv_math == 'bf16' (bf16 storage between the convolutions)."""
    return Dims(S, V, T, R, E, units, blocks, backbone_from, compute_dtype, bool(conv_bf16))


def configs4_dims(d):
    """BASELINE configs[4]'s own size (bench.py --config joint: 1024 px, 200 RoIs, 15 tokens, V = 50 000) in d's mode.  The stage-4 block
    count stays d's: the blocks of a stage are the same layer shapes again, so the count adds names, not routing decisions.
    What planned_sites compares between two sizes are the PRODUCTS' pipes.  Two limits: (1) the rounding of the vocabulary layer's logits
    (role 'out', dc_vocab_ce's materialize_bf16) is not in the site model -- the library decides it from its tile cost model
    (b256::prefer), which it does not export; configs[4]'s size takes it, the parity tests' sizes never do; (2) RoiHead._mm's use_b,
    CaptionModelV1's emb_b / du_b and EncoderPlan._conv's storage test are restated in planned_sites (they are inline in the package), and
    the recorder checks the restatement against the device at the TEST's size only: at configs[4]'s size it is as good as the copy."""
    return d._replace(S=1024, V=50000, T=15, R=200)


def group_of(name):
    layer = name.split("/")[0].split(":")[0].split(".")[0].split("@")[0]
    if layer.startswith("imgcap_"):
        return "decoder"
    if layer.startswith("mrcnn_"):
        return "head"
    if layer.startswith(("fpn_", "rpn_")):
        return "fpn_rpn"
    return "trunk"


def _fused(site):
    layer, _, rest = site.partition("@")
    return FUSED.get(layer, layer) + ("@" + rest if rest else "")


def _mm_on_bf16(d, M, N, K, a_stride, w_stride, a_trans=False, b_trans=False):
    """RoiHead._mm's use_b (text_generation_model.py) for a weight that has a bf16 mirror or an activation operand."""
    return (d.compute_dtype == "bf16" and K % 8 == 0 and a_stride % 8 == 0 and w_stride % 8 == 0 and
            (not a_trans or M % 8 == 0) and (b_trans or N % 8 == 0))


def planned_sites(d):
    """{site: Site} of one train step of DenseImageCapRCNN(compute_dtype=d.compute_dtype, conv_math='bf16' if d.conv_bf16 else default),
    trainable ResNet stages >= d.backbone_from.  Recurrent dropout off, one mask set per RoI (the parity tests' graph)."""
    from image_captioning_amd import ops
    from image_captioning_amd.layers import resnet_fpn_convs
    bf = d.compute_dtype == "bf16"
    R, T, V, E, u = d.R, d.T, d.V, d.E, d.units
    N = T * R
    K1 = POOL * POOL * FPN_C
    Ep = (E + 7) // 8 * 8
    sites = {}

    def mm(site, M, Nn, K, a_stride, w_stride, a_trans=False, b_trans=False):
        sites[site] = Site("gemm", _mm_on_bf16(d, M, Nn, K, a_stride, w_stride, a_trans, b_trans), tuple(sorted((M, Nn, K))))

    # ---- RoI head (RoiHead._head_forward / _head_backward): every product through _mm
    for name, k in (("mrcnn_class_conv1", K1), ("mrcnn_class_conv2", FEAT)):
        mm(name + ":fwd", R, FEAT, k, k, FEAT)
        mm(name + ":wgrad", k, FEAT, R, k, FEAT, a_trans=True)
        mm(name + ":dgrad", R, k, FEAT, FEAT, FEAT, b_trans=True)
    # ---- decoder forward (CaptionModelV1._hidden)
    emb_b = bf and Ep <= E + FEAT                                   # _emb_bf16: the padded table fits the kernel's rows
    mm("imgcap_lstm1.feat:fwd", R, 4 * u, FEAT, FEAT, 4 * u)
    sites["imgcap_lstm1.emb:fwd"] = Site("gemm", emb_b, tuple(sorted((N, 4 * u, Ep if emb_b else E))))
    mm("imgcap_lstm2:fwd", N, 4 * u, u, u, 4 * u)
    mm("imgcap_lstm_d1.feat:fwd", R, D1, FEAT, FEAT, D1)
    mm("imgcap_lstm_d1.h:fwd", N, D1, u, u, D1)
    a1_b = sites["imgcap_lstm_d1.h:fwd"].bf16                      # want_b: the bf16 copy of a1 exists only when that GEMM ran on the bf16 pipe
    X, W = _Shape((N, D1), bf16=True), _Shape((D1, V), bf16=True)
    vocab_b = bool(bf and a1_b and N % 8 == 0 and ops.vocab_ce_supported(X, W))
    sites["imgcap_lstm_d2:fwd"] = Site("vocab", vocab_b, (N, V, D1))
    # ---- decoder backward (CaptionModelV1._backward): dl.f is None <=> the fused loss wrote a bf16 gradient
    sites["imgcap_lstm_d2:wgrad"] = Site("gemm", vocab_b, tuple(sorted((D1, V, N))))
    sites["imgcap_lstm_d2:dgrad"] = Site("gemm", vocab_b, tuple(sorted((N, D1, V))))
    mm("imgcap_lstm_d1.h:wgrad", u, D1, N, u, D1, a_trans=True)
    mm("imgcap_lstm_d1.feat:wgrad", FEAT, D1, R, FEAT, D1, a_trans=True)
    mm("imgcap_lstm_d1.feat:dgrad", R, FEAT, D1, D1, D1, b_trans=True)
    mm("imgcap_lstm_d1.h:dgrad", N, u, D1, D1, D1, b_trans=True)
    du_b = vocab_b and bf and T > 1 and ((T - 1) * R) % 8 == 0 and u % 8 == 0
    for l in ("imgcap_lstm1", "imgcap_lstm2"):
        sites[l + ".rec:wgrad"] = Site("gemm", du_b, tuple(sorted((u, 4 * u, (T - 1) * R))))
    mm("imgcap_lstm2:wgrad", u, 4 * u, N, u, 4 * u, a_trans=True)
    mm("imgcap_lstm2:dgrad", N, u, 4 * u, 4 * u, 4 * u, b_trans=True)
    emb_w = vocab_b and emb_b and N % 8 == 0
    sites["imgcap_lstm1.emb:wgrad"] = Site("gemm", emb_w, tuple(sorted((Ep if emb_w else E, 4 * u, N))))
    mm("imgcap_lstm1.feat:wgrad", FEAT, 4 * u, R, FEAT, 4 * u, a_trans=True)
    mm("imgcap_lstm1.feat:dgrad", R, FEAT, 4 * u, 4 * u, 4 * u, b_trans=True)
    # ---- convolutions.  Forward (EncoderPlan._conv): bf16 storage takes every layer with Cin % 64 == 0; what it does not take (the stem)
    # runs the fp32-storage kernel in DC_MATH_BF16 = both operands rounded once: the same arithmetic, so the same kind of site
    specs = {s.name: s for s in resnet_fpn_convs(d.blocks)}
    size = {"conv1": d.S // 2}
    for s in specs.values():
        if s.name.startswith("res"):
            size[s.name] = d.S // {2: 4, 3: 8, 4: 16, 5: 32}[int(s.name[3])]
    for k in (2, 3, 4, 5, 6):
        size["fpn_c%dp%d" % (k, k)] = size["fpn_p%d" % k] = size["@P%d" % k] = d.S // 2 ** k
    train_from = d.backbone_from

    def stage_of(name):
        return 1 if name == "conv1" else int(name[3]) if name.startswith("res") else None

    def conv_sites(site, s, hw):
        fwd_b = d.conv_bf16                               # (every layer of the plan, the stem through DC_MATH_BF16)
        sites[site + ":fwd"] = Site("conv", fwd_b, (hw, s.k, s.cin, s.cout))
        st = stage_of(s.name)
        trained = st is None or (train_from is not None and st >= train_from)
        if not trained:
            return
        w_b = bool(bf and s.stride == 1 and s.name not in ("rpn_head", "conv1") and ops.wgrad_bf16_supported((1, hw, hw, s.cin), (1, hw, hw, s.cout)))
        sites[site + ":wgrad"] = Site("wgrad", w_b, (hw, s.k, s.cin, s.cout))
        d_b = bool(d.conv_bf16 and s.k == 3 and s.stride == 1 and ops.conv_bf16_supported(s.cout))      # _dgrad: the 3x3 layers; 1x1 data gradients are fp32 GEMMs
        sites[site + ":dgrad"] = Site("conv", d_b, (hw, s.k, s.cout, s.cin))

    for s in specs.values():
        conv_sites(s.name, s, size[s.name])
    Spec = collections.namedtuple("Spec", "name k cin cout stride")
    for k in (2, 3, 4, 5, 6):
        conv_sites("rpn_conv_shared@P%d" % k, Spec("rpn_conv_shared", 3, FPN_C, 512, 1), size["@P%d" % k])
        conv_sites("rpn_head@P%d" % k, Spec("rpn_head", 1, 512, 0, 1), size["@P%d" % k])
    return sites


def inference_sites(d):
    """The forward products of the inference graph with the reference's prefix decoder (CaptionModelV1.generate): the training forward's,
    except that the vocabulary layer scores words from the fp32 activations and the fp32 master weight (ops.gemm)."""
    sites = {s: v for s, v in planned_sites(d).items() if s.endswith(":fwd")}
    sites["imgcap_lstm_d2:fwd"] = sites["imgcap_lstm_d2:fwd"]._replace(kind="gemm", bf16=False)
    return sites


class _Shape(object):
    """What ops.vocab_ce_supported reads of a contiguous 2-D tensor."""

    def __init__(self, shape, bf16):
        import torch
        self.shape, self.dtype = tuple(shape), torch.bfloat16 if bf16 else torch.float32

    def stride(self, i):
        return self.shape[1] if i == 0 else 1


def bf16_set(sites):
    return {k for k, s in sites.items() if s.bf16}


class Bf16Policy(object):
    """quant(site, role, array) for the oracle: O.to_bf16 (after a cast to float32, as the device holds fp32) at the sites of `on_bf16`,
    the array itself elsewhere.  known: every site the step has (planned_sites' keys); a site outside it is an error -- the oracle and
    the plan must name the same products.  materialise: the vocabulary layer's logits are stored in bf16 and read back (role 'out';
    dc_vocab_ce's materialize_bf16, which the library takes on the 256-square tile only: never at the parity tests' sizes)."""
    OPERANDS = ("x", "w", "dy")
    # A handed-over copy g of an operand a (below) must be a rounding the device could have made of ITS fp32 value of a: within half a bf16
    # ulp of a, plus REACH x max|a| for what fp32 accumulation (sums of up to 12 544 terms: sqrt(K) u ~ 7e-6 typical, K u = 7.5e-4 worst case)
    # moves the device's value away from the float64 one -- 2^-13, between the two; and it may differ from the oracle's own rounding in at
    # most FLIP_CAP of the entries (an entry flips when the two values straddle a rounding boundary: reach / ulp of the entries, ~1 %).
    REACH = 2.0 ** -13
    FLIP_CAP = 0.02

    CUT_TOL = 4e-3                     # a cut input against the oracle's own value, relative L2: 4 x the 1.0e-3 measured at C3 (the size of the rounding step)

    def __init__(self, on_bf16, known=None, materialise=False, given=None, pool=None, cuts=None):
        """given = {(site, role): array}: the bf16 copies of activation / gradient operands the device (or its stand-in) formed, in the
        oracle's layout.  Which of its two bf16 neighbours an operand is rounded to is a discrete decision like a ReLU's sign; a chain
        of products that each read rounded operands amplifies a difference of one fp32 ulp to the size of the rounding step itself within
        a few layers (an entry that flips moves by a whole bf16 ulp: error e -> sqrt(e ulp) per layer).  So the decision is checked
        (it is a legitimate rounding of the oracle's value, see REACH) and handed to the oracle, as _parity_cuts does for the head's
        ReLU masks; .handed records, per operand, how many entries differ from the oracle's own rounding and the worst violation."""
        self.on, self.known, self.materialise = {_fused(s) for s in on_bf16}, None if known is None else set(known), bool(materialise)
        self.rounded = collections.defaultdict(set)            # site -> operand roles rounded
        self.seen = set()
        self._w = {}
        self.members = collections.defaultdict(lambda: collections.defaultdict(set))      # fused site -> oracle site -> operand roles rounded
        self.given = dict(given or {})
        # pool = [array]: the bf16 operand copies of the device's convolution launches (SiteRecorder.pool) without a name: an operand the
        # oracle is about to round takes the copy of its shape that lies nearest, and the same check decides whether it is one.
        # cuts = {(site, role): array}: the device's value of an INPUT of the compared part (the output of a frozen stage, whose inner
        # activations are recycled and cannot be handed over): compared with the oracle's own at CUT_TOL (.cut_errs) and used as it is,
        # on either pipe -- the comparison behind it holds the part from that input on (tests/_parity_cuts.py, rule 1).
        self.pool = collections.defaultdict(list)
        for t in (pool or ()):
            self.pool[tuple(np.shape(t))].append(np.asarray(t, np.float64))
        self.cuts, self.cut_errs = dict(cuts or {}), {}
        self.upstream = ("\0",)                                # name prefixes of the sites in front of the cuts: the oracle rounds those itself
        self.handed = {}                                       # (site, role) -> dict(flips, size, excess)

    @classmethod
    def planned(cls, d, materialise=False):
        sites = planned_sites(d)
        return cls(bf16_set(sites), known=sites, materialise=materialise)

    def __call__(self, site, role, a):
        raw, site = site, _fused(site)
        if role in self.OPERANDS and site in self.on:
            self.members[site][raw].add(role)
        if self.known is not None and site not in self.known:
            raise KeyError("the oracle names a product site the plan does not know: %r" % site)
        self.seen.add(site)
        if role == "out":
            return O.to_bf16(a) if self.materialise and site in self.on else a
        if role not in self.OPERANDS:
            raise ValueError("role %r" % role)
        cut = self.cuts.get((site, role))
        if cut is not None:
            cut = np.asarray(cut, np.float64).reshape(np.shape(a))
            self.cut_errs[(site, role)] = l2_err(cut, O.to_bf16(a) if site in self.on else a)
            if site in self.on:
                self.rounded[site].add(role)
            return cut
        if site not in self.on:
            return a
        self.rounded[site].add(role)
        if role != "w":
            own = O.to_bf16(a)
            g = self.given.get((raw, role))
            if g is None and not site.startswith(self.upstream):
                cands = self.pool.get(tuple(np.shape(a)))
                if cands:
                    a64 = np.asarray(a, np.float64)
                    g = min(cands, key=lambda c: float(np.abs(c - a64).mean()))
            return own if g is None else self._hand_over(raw, role, np.asarray(a, np.float64), own, g)
        # a kernel is rounded once per policy (forward and data gradient read the same copy; the head's first kernel has 12.8 M entries):
        # a policy serves ONE weight dict
        key = (site.rsplit(":", 1)[0], np.shape(a))
        if key not in self._w:
            self._w[key] = O.to_bf16(a)
        return self._w[key]

    def _hand_over(self, site, role, a, own, g):
        g = np.asarray(g, np.float64).reshape(a.shape)
        with np.errstate(divide="ignore"):
            half_ulp = np.where(a == 0, 0.0, 2.0 ** (np.floor(np.log2(np.abs(np.where(a == 0, 1.0, a)))) - 8))
        scale = float(np.abs(a).max())
        excess = float((np.abs(g - a) - half_ulp).max() / max(scale, 1e-300))            # in units of max|a|: must stay below REACH
        on_grid = bool(np.array_equal(O.to_bf16(g), g))
        h = self.handed[(site, role)] = dict(flips=int((g != own).sum()), size=int(a.size), excess=excess, on_grid=on_grid)
        ok = on_grid and excess <= self.REACH and h["flips"] <= self.FLIP_CAP * h["size"]
        return g if ok else own                                # a copy that is no rounding of this value is reported (handed_violations), not used

    def handed_violations(self):
        """Handed-over operands that are not legitimate roundings of the oracle's values: [(site, role, record)]."""
        return [(s, r, h) for (s, r), h in sorted(self.handed.items())
                if not h["on_grid"] or h["excess"] > self.REACH or h["flips"] > self.FLIP_CAP * h["size"]]

    def rounded_products(self):
        """Sites at which both operands were rounded; a fused site (rpn_head = rpn_class_raw + rpn_bbox_pred) only if that holds for every
        one of its oracle products that was evaluated."""
        return sorted(s for s, r in self.rounded.items() if len(r) >= 2 and all(len(m) >= 2 for m in self.members[s].values()))


class Float32StandIn(Bf16Policy):
    """The device stood in for on the CPU (tests/test_bf16_sites.py): the same rounding, every product in np.float32 (the hook's dtype
    carries through the oracle's products), activations cast to float32 before they are rounded.  Planted errors:
    unrounded = {(site, role)}: that operand is read unrounded (a site on the fp32 pipe: both of its operands);
    scale_dy = {site: factor}: the gradient operand of that site is scaled before it is rounded."""

    def __init__(self, on_bf16, known=None, materialise=False, unrounded=(), scale_dy=None):
        Bf16Policy.__init__(self, on_bf16, known, materialise)
        self.unrounded, self.scale_dy = set(unrounded), dict(scale_dy or {})
        self.made = {}                                         # (site, role) -> the activation / gradient operand copies it formed: the oracle's `given`

    def __call__(self, site, role, a):
        a = np.asarray(a, np.float32)
        if role == "dy" and site in self.scale_dy:
            a = a * np.float32(self.scale_dy[site])
        out = a if (site, role) in self.unrounded else np.asarray(Bf16Policy.__call__(self, site, role, a), np.float32)
        if role in ("x", "dy") and _fused(site) in self.on:
            self.made[(site, role)] = out
        return out


class SiteRecorder(Recorder):
    """Recorder + (name, shapes) of every top-level launch of the product kernels, split by pipe: .bf16 and .f32 lists of (kind, op, shapes)."""
    KINDS = {"gemm_bf16": "gemm", "gemm": "gemm", "conv2d_bf16": "conv", "conv2d": "conv", "conv2d_wgrad_bf16": "wgrad", "conv2d_wgrad": "wgrad",
             "vocab_ce": "vocab"}

    def __init__(self, model):
        Recorder.__init__(self, model)
        self.bf16, self.f32 = [], []
        self.pool = []                                         # copies of the bf16 activation / gradient operands of the convolution launches

    def _wrap(self, name, fn):
        inner = Recorder._wrap(self, name, fn)
        if name not in self.KINDS:
            return inner

        def call(*a, **k):
            if self.depth == 0:
                import torch
                on_b = a[0].dtype == torch.bfloat16
                (self.bf16 if on_b else self.f32).append((self.KINDS[name], name, tuple(tuple(t.shape) for t in a[:2])))
                if on_b and name in ("conv2d_bf16", "conv2d_wgrad_bf16"):          # (x, dy) of a weight gradient; dy of a data gradient (its kernel is a weight)
                    self.pool.extend(t.clone() for t in (a[:2] if name == "conv2d_wgrad_bf16" else a[:1]))
            return inner(*a, **k)
        return call

    def add_plan_forward(self, plan):
        """The plan's forward convolutions (EncoderPlan._ops: launched by the plan itself, replayed from a captured graph after the first
        pass): 'bconv' = dc_conv2d_bf16; 'conv' with DC_MATH_BF16 = the fp32-storage kernel on operands rounded once."""
        from image_captioning_amd import _lib
        for op in plan._ops:
            if op[0] == "bconv" or (op[0] == "conv" and op[1].math == _lib.MATH_BF16):
                self.bf16.append(("conv", "plan:" + op[2], ()))
            elif op[0] in ("conv", "chain"):
                self.f32.append(("conv", "plan:" + op[2], ()))
        self.pool.extend(plan._twin.values())                  # the bf16 twins of the plan's buffers: what its bf16 convolutions read

    def pool_arrays(self):
        """The pool as float64 host arrays, one per distinct content."""
        seen, out = set(), []
        for t in self.pool:
            a = t.float().cpu().numpy()
            key = (a.shape, a.tobytes())
            if key not in seen:
                seen.add(key)
                out.append(a.astype(np.float64))
        return out

    def plan_bf16_layers(self):
        return sorted(n[5:] for _, n, _ in self.bf16 if n.startswith("plan:"))


def check_sites(rec, policy, sites):
    """The device's bf16-pipe launches (rec: a SiteRecorder of the step, plan forward added) against the products the policy rounded in the
    oracle's evaluation of the same step: the same number, kind by kind; every planned bf16 site was rounded and nothing else."""
    want = bf16_set(sites)
    got = set(policy.rounded_products())
    by_kind = lambda items: dict(collections.Counter(items))
    dev, ora = by_kind(k for k, _, _ in rec.bf16), by_kind(sites[s].kind for s in got)
    ok = got == want and dev == ora and len(rec.bf16) == len(got)
    if not ok:
        print("bf16-pipe launches of the device (%d): %s" % (len(rec.bf16), dev))
        for r in rec.bf16:
            print("   ", r)
        print("fp32 launches beside them (%d):" % len(rec.f32))
        for r in rec.f32:
            print("   ", r)
        print("products the oracle rounded (%d): %s" % (len(got), ora))
        for s in sorted(got):
            print("   ", s, sites[s])
        print("planned but not rounded:", sorted(want - got), " rounded but not planned:", sorted(got - want))
    assert got == want, "the oracle rounded %d products, the plan puts %d on the bf16 pipe" % (len(got), len(want))
    assert len(rec.bf16) == len(got) and dev == ora, "%d launches on the bf16 pipe %s, %d rounded oracle products %s" % (len(rec.bf16), dev, len(got), ora)
    fwd = rec.plan_bf16_layers()
    if fwd:
        planned_fwd = sorted(_fused(s[:-4]).split("@")[0] for s in want if s.endswith(":fwd") and sites[s].kind == "conv")
        assert fwd == planned_fwd, (sorted(set(fwd) - set(planned_fwd)), sorted(set(planned_fwd) - set(fwd)))
    return len(got)


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------------------

def l2_err(got, want):
    want = np.asarray(want, np.float64)
    return float(np.linalg.norm(np.asarray(got, np.float64) - want) / max(1e-30, np.linalg.norm(want)))


def compare(got, want, keys=None):
    """{tensor: relative L2 error} over `keys` (default: want's); a tensor the oracle holds at exactly zero (dead units) must be zero."""
    out = {}
    for k in (want if keys is None else keys):
        w = np.asarray(want[k], np.float64)
        if np.abs(w).max() <= 1e-12:
            assert np.abs(np.asarray(got[k], np.float64)).max() < 1e-9, k
            continue
        out[k] = l2_err(got[k], w)
    return out


def worst_per_group(errs):
    out = {}
    for k, v in errs.items():
        g = group_of(k)
        out[g] = max(out.get(g, 0.0), v)
    return out


def failures(errs, tol):
    """Tensors above their group's tolerance (tol: {group: value}), worst first."""
    bad = [(k, v) for k, v in errs.items() if not np.isfinite(v) or v >= tol[group_of(k)]]
    return sorted(bad, key=lambda kv: -kv[1] if np.isfinite(kv[1]) else -np.inf)


def assert_close(errs, tol, what=""):
    bad = failures(errs, tol)
    print("%s worst per group: %s" % (what, {g: "%.3g" % v for g, v in sorted(worst_per_group(errs).items())}))
    assert not bad, "%s %d tensor(s) above tolerance %s; worst: %s" % (what, len(bad), tol, [(k, "%.3g" % v) for k, v in bad[:8]])


def report(name, errs, lerrs, n_sites):
    """Every figure of one comparison on stdout, before anything is asserted on it: one line per tensor group and one JSON line
    (profiles/bf16_step_parity.json is made of these)."""
    import json
    print("%s: %d products on the bf16 pipe; losses %s" % (name, n_sites, {k: "%.3g" % v for k, v in sorted(lerrs.items())}))
    for k, v in sorted(errs.items(), key=lambda kv: -kv[1])[:8]:
        print("    %-40s %.3g" % (k, v))
    print("BF16_PARITY " + json.dumps({"name": name, "sites": n_sites, "losses": lerrs, "tensors": errs}, sort_keys=True))


# Tolerances of the GPU comparisons against the rounding oracle: 4 x the largest figure measured on the MI355X in each group, rounded up to
# one significant digit -- the margin is for another build's accumulation order (DESIGN.md section 3d holds the measured figures, the CPU
# floor and the planted-error figures beside them; tests/test_bf16_sites.py asserts that each value is below half of what the planted
# errors do to the tensors they touch).
#   train step, compute_dtype='bf16' (roundings of the head's and the decoder's operands handed over), MEASURED:
#     decoder 7.33e-8 (imgcap_lstm1/bias)   head 1.12e-7 (mrcnn_class_bn1/gamma)   fpn_rpn 6.77e-7 (rpn_bbox_pred/kernel)   losses 1.04e-7 (rpn_class_loss)
TOL_STEP = {"decoder": 3e-7, "head": 5e-7, "fpn_rpn": 3e-6, "losses": 5e-7}
#   train step, compute_dtype='bf16' + conv_math='bf16', stages 4+ / all trainable (every operand rounding of the compared part handed over,
#   frozen stages cut at their outputs), MEASURED, the larger of the two cases:
#     trunk 3.42e-7 (conv1/kernel)   fpn_rpn 2.76e-7 (rpn_bbox_pred/kernel)   decoder 7.79e-8   head 1.22e-7   losses 8.52e-8 (imgcap_loss)
TOL_TRUNK_STEP = {"decoder": 4e-7, "head": 5e-7, "fpn_rpn": 2e-6, "trunk": 2e-6, "losses": 4e-7}
#   inference forward (tests/test_gpu_models.py::test_joint_model_inference_in_bf16), MEASURED: see below
#     pyramid 3.44e-3 (the device's P2..P5 against the rounding oracle's own: ~40 layers that each read rounded stored activations, which the
#     inference plan recycles -- the size of the rounding step, a cut input like Bf16Policy.CUT_TOL);  behind the cut: RoI features 3.36e-8
#     (relative L2, against RoIAlign of the device's maps), log-probabilities 5.14e-7 (largest |difference|, roundings handed over)
TOL_INFERENCE = {"pyramid": 2e-2, "features": 2e-7, "logprobs": 3e-6}


def loss_errs(got, want, keys=("imgcap_loss", "rpn_class_loss", "rpn_bbox_loss", "reg_loss", "loss")):
    return {k: abs(float(got[k]) - float(want[k])) / max(1.0, abs(float(want[k]))) for k in keys}


# ---------------------------------------------------------------------------------------------------------------------------------
# one device step against the rounding oracle
# ---------------------------------------------------------------------------------------------------------------------------------

def device_roundings(top, R, T):
    """{(site, role): array}: the bf16 copies of the activations and gradients the head and the decoder multiplied in the step `top` (a
    CaptionModelV1 that computes in bf16) has just run, in the oracle's layout ([R,T,.] where the device holds time-major rows t*R+b).
    They are the operand buffers of RoiHead._mm (_Act.b: '<key>:bf16'), the Dense-1024 epilogue's copy 'a1:outb' and the fused loss's
    bf16 gradient; weights and the embedding rows are not handed over (both sides round the same fp32 values)."""
    bufs = top._bufs
    host = lambda key: bufs[key].float().cpu().numpy().astype(np.float64)
    tm = lambda a: a.reshape(T, R, -1).transpose(1, 0, 2)
    prev = lambda a: np.concatenate([np.zeros_like(a[:, :1]), a[:, :-1]], axis=1)
    X, hact0, f = host('X:bf16'), host('hact0:bf16'), host('hact1:bf16')
    h1, h2, a1 = tm(host('h1:bf16')), tm(host('h2:bf16')), tm(host('a1:outb'))
    dlog = tm(host('dlogits:bf16')[:, :top.V])
    dz_d1, dzd_f = tm(host('dz_d1:bf16')), host('dzd_f:bf16')
    dz2, dz1, dzf = tm(host('dz2:bf16')), tm(host('dz1:bf16')), host('dzf:bf16')
    dacc1, dacc0 = host('dacc1:bf16'), host('dacc0:bf16')
    g = {}
    for site, role, a in (
            ('mrcnn_class_conv1:fwd', 'x', X), ('mrcnn_class_conv1:wgrad', 'x', X), ('mrcnn_class_conv2:fwd', 'x', hact0), ('mrcnn_class_conv2:wgrad', 'x', hact0),
            ('imgcap_lstm1.feat:fwd', 'x', f), ('imgcap_lstm_d1.feat:fwd', 'x', f), ('imgcap_lstm1.feat:wgrad', 'x', f), ('imgcap_lstm_d1.feat:wgrad', 'x', f),
            ('imgcap_lstm2:fwd', 'x', h1), ('imgcap_lstm2:wgrad', 'x', h1), ('imgcap_lstm1.rec:wgrad', 'x', prev(h1)),
            ('imgcap_lstm_d1.h:fwd', 'x', h2), ('imgcap_lstm_d1.h:wgrad', 'x', h2), ('imgcap_lstm2.rec:wgrad', 'x', prev(h2)),
            ('imgcap_lstm_d2:fwd', 'x', a1), ('imgcap_lstm_d2:wgrad', 'x', a1),
            ('imgcap_lstm_d2:wgrad', 'dy', dlog), ('imgcap_lstm_d2:dgrad', 'dy', dlog),
            ('imgcap_lstm_d1.h:wgrad', 'dy', dz_d1), ('imgcap_lstm_d1.h:dgrad', 'dy', dz_d1),
            ('imgcap_lstm_d1.feat:wgrad', 'dy', dzd_f), ('imgcap_lstm_d1.feat:dgrad', 'dy', dzd_f),
            ('imgcap_lstm2.rec:wgrad', 'dy', dz2), ('imgcap_lstm2:wgrad', 'dy', dz2), ('imgcap_lstm2:dgrad', 'dy', dz2),
            ('imgcap_lstm1.rec:wgrad', 'dy', dz1), ('imgcap_lstm1.emb:wgrad', 'dy', dz1),
            ('imgcap_lstm1.feat:wgrad', 'dy', dzf), ('imgcap_lstm1.feat:dgrad', 'dy', dzf),
            ('mrcnn_class_conv2:wgrad', 'dy', dacc1), ('mrcnn_class_conv2:dgrad', 'dy', dacc1),
            ('mrcnn_class_conv1:wgrad', 'dy', dacc0), ('mrcnn_class_conv1:dgrad', 'dy', dacc0)):
        g[(site, role)] = a
    return g


def assert_handed_over(policy, expect):
    """Every operand of `expect` ({(site, role)}) was handed over, and each is a legitimate rounding of the oracle's value (Bf16Policy.REACH,
    FLIP_CAP)."""
    missing = sorted(set(expect) - set(policy.handed))
    assert not missing, "operands the oracle never asked for: %s" % missing
    flips = sum(h["flips"] for h in policy.handed.values())
    size = sum(h["size"] for h in policy.handed.values())
    worst = max(policy.handed.values(), key=lambda h: h["excess"])
    print("handed-over roundings: %d operands, %d of %d entries rounded to the other neighbour, worst excess %.3g of max|a| (reach %.3g)"
          % (len(policy.handed), flips, size, worst["excess"], policy.REACH))
    if policy.cut_errs:
        print("cut inputs against the oracle's own: %s" % {k[0]: "%.3g" % v for k, v in sorted(policy.cut_errs.items())})
        assert set(policy.cut_errs) == set(policy.cuts) and max(policy.cut_errs.values()) < policy.CUT_TOL, policy.cut_errs
    bad = policy.handed_violations()
    assert not bad, "handed-over operands that are no rounding of the oracle's value: %s" % bad[:6]


def frozen_stage_cuts(plan, d):
    """The cuts of a step whose ResNet stages below d.backbone_from are frozen (their inner activations are recycled): the stage outputs
    the compared part reads -- C_{from-1} as the input of stage `from`'s entry convolutions, and every frozen C_k as the input of its FPN
    lateral -- as the device holds them: the bf16 twin for a product on the bf16 pipe, the fp32 map for one on the fp32 pipe."""
    cuts = {}
    low = d.backbone_from if d.backbone_from is not None else 6
    host = lambda t: t.float().cpu().numpy().astype(np.float64)
    sites = planned_sites(d)
    for k in (2, 3, 4, 5):
        if k >= max(low, 2):
            continue
        c = plan.C[k - 2]
        f32, b16 = host(c), host(plan.bf16_of(c))
        names = ["fpn_c%dp%d:fwd" % (k, k), "fpn_c%dp%d:wgrad" % (k, k)]
        if k == low - 1:
            names += ["res%da_branch%s:%s" % (low, br, ph) for br in ("2a", "1") for ph in ("fwd", "wgrad")]
        for n in names:
            cuts[(n, "x")] = b16 if sites[n].bf16 else f32
    return cuts


def rounded_step(model, Wt, ocfg, inputs, tg, d, rec, hand_over=True):
    """The rounding oracle's evaluation of the step `model` has just run (its forward_backward recorded by `rec`, a SiteRecorder), on the
    RoI sample the device drew (tg = model.last_targets), the head's two ReLU decisions the device took and the roundings of the head's
    and the decoder's activation and gradient operands it made (device_roundings).  Returns a dict: sites, policy, want (losses), G
    (gradients), aux, dev_acc / dev_hact (the device's head buffers), given -- all read BEFORE anything else runs on the model.
    hand_over=False: the oracle rounds every operand itself (a step whose RoI features already differ from the oracle's by a rounding step:
    bf16 storage between the convolutions)."""
    from oracle import np_models as M
    import _parity_cuts as PC
    img, _, match, tdelta, gt_caps, gt_boxes = inputs[:6]
    sites = planned_sites(d)
    given = device_roundings(model.caption_model, d.R, d.T) if hand_over else {}
    dev_acc, dev_hact = PC.device_head_buffers(model.caption_model)
    rec.add_plan_forward(model.plan())
    cuts = frozen_stage_cuts(model.plan(), d) if (hand_over and d.conv_bf16) else {}
    policy = Bf16Policy(bf16_set(sites), known=sites, given=given, pool=rec.pool_arrays() if hand_over else None, cuts=cuts)
    if cuts:
        policy.upstream = ("conv1",) + tuple("res%d" % k for k in range(2, d.backbone_from))
    want, G, aux = M.joint_loss_and_grads(Wt, img[0], match[0, :, 0], tdelta[0], gt_caps[0], gt_boxes[0], ocfg, stage4_blocks=d.blocks,
                                          targets_override=(tg['rois'], tg['caps']), backbone_from=d.backbone_from,
                                          head_masks=PC.device_head_masks(dev_hact), quant=policy)
    return dict(sites=sites, policy=policy, want=want, G=G, aux=aux, dev_acc=dev_acc, dev_hact=dev_hact, given=given)
