"""Stacked hourglass on the HIP kernels (H1-H6).

Drop-in for StackedHourglass / pose_model / PoseModel
(models/pose/hourglass.py:7-99, models/pose/pose_model.py:5-13,
models/__init__.py:4):

* the module tree, parameter names and order, buffer names, shapes and the
  default initialisation are the reference's (so torch.manual_seed(s) gives
  bit-identical weights, and state_dict() interchanges with reference
  checkpoints);
* every parameter is an alias into ONE flat device buffer (`flat_params`,
  grad-carrying parameters first, the never-trained skip_layer parameters of
  identity Residuals last), gradients accumulate into `flat_grads`, BN
  running statistics live in `flat_stats` — so the EMA teacher update, the
  optimizer step and the DDP all-reduce are each a single kernel / collective
  over a contiguous buffer;
* forward/backward are explicit executors over the HIP kernels (the conv*.hip files with
  the pre-activation BN+ReLU fused into operand staging, bn_fwd.hip / bn_bwd.hip, pool.hip);
  autograd sees the whole network as one Function.

The parameter table, its initialisation and the weight tables / weight set are in
hourglass_params.py, the executor (`_Exec`) and its two environment switches in
hourglass_exec.py; this module holds the model and its autograd Function.
"""
import torch
from torch import nn

from . import _lib
from . import kernels as Kn
from .hourglass_exec import BN_EPS, BN_MOMENTUM, _FP16_BWD3, _Exec  # noqa: F401  (BN_*: re-exported)
from .hourglass_params import _Node, _WeightSet, _default_init, build_table, build_weight_tables


class StackedHourglass(nn.Module):
    """StackedHourglass(k, nStack, mode) on the HIP path.  forward(imgs) ->
    preds [B,S,K,R,R] (mode 'default') or (preds, features [B,S,256,R/2,R/2])
    for mode 'AvgPool' / 'MaxPool' (models/pose/hourglass.py:60-99).  'ConvOne'
    builds a 128-channel conv on 256-channel features in the reference and
    fails there; it is rejected here."""

    def __init__(self, k, nStack, mode="default", device=None):
        super().__init__()
        if mode not in ("default", "AvgPool", "MaxPool"):
            raise ValueError("mode %r unsupported (ConvOne is broken in the reference: hourglass.py:227)" % mode)
        _lib.require_gpu()
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.k, self.nStack, self.mode = k, nStack, mode
        tab = build_table(k, nStack)
        vals = _default_init(tab)          # CPU RNG, reference order
        # flat layout: live parameters first (reference order), dead ones last
        order = [i for i, e in enumerate(tab) if e[3]] + [i for i, e in enumerate(tab) if not e[3]]
        offs, o = {}, 0
        for i in order:
            n = vals[i].numel()
            offs[tab[i][0]] = (o, n, tab[i][1])
            o += (n + 3) // 4 * 4          # keep every segment 16-B aligned
        self.n_total = o
        self.n_live = max(offs[tab[i][0]][0] + offs[tab[i][0]][1] for i in order if tab[i][3])
        self.n_live = (self.n_live + 3) // 4 * 4
        host = torch.zeros(self.n_total)
        for i, e in enumerate(tab):
            s, n, _ = offs[e[0]]
            host[s:s + n] = vals[i].reshape(-1)
        self.flat_params = host.to(device)
        self.flat_grads = torch.zeros(self.n_total, device=device)
        self._offs = offs
        self._table = tab
        # BN running statistics in one flat buffer: per BN [mean(C) | var(C)]
        bns = [e[0][:-len(".weight")] for e in tab if e[2] == "bw"]
        self._bn_names = bns
        so, sidx = 0, {}
        for b in bns:
            c = offs[b + ".weight"][1]
            sidx[b] = (so, c)
            so += 2 * c
        stats = torch.zeros(so)
        for b, (s, c) in sidx.items():
            stats[s + c:s + 2 * c] = 1.0
        self.flat_stats = stats.to(device)
        self._nbt = torch.zeros(len(bns), dtype=torch.long, device=device)
        self._sidx = sidx
        self._bn_index = {b: i for i, b in enumerate(bns)}
        # module tree with aliased parameters / buffers, in reference order
        for name, shape, kind, _ in tab:
            mod, attr = self._node_for(name)
            s, n, shp = offs[name]
            mod.register_parameter(attr, nn.Parameter(self.flat_params[s:s + n].view(shp)))
            if kind == "bb":
                b = name[:-len(".bias")]
                bs, c = sidx[b]
                mod.register_buffer("running_mean", self.flat_stats[bs:bs + c])
                mod.register_buffer("running_var", self.flat_stats[bs + c:bs + 2 * c])
                mod.register_buffer("num_batches_tracked", self._nbt[self._bn_index[b]])
        self._grad_views_attached = False
        self._ws = {}
        self._grad_keep = []          # upstream gradients alive until their stream is joined
        # re-laid-out conv weights, rebuilt by one launch per forward (tap-major
        # [Cout][T][Cin] for KS > 1) and per backward (dgrad [Cin][T][Cout]):
        # tables per conv precision, see set_conv_precision / hourglass_params.build_weight_tables
        self._device = device
        self.set_conv_precision(None)

    # -- structure helpers ------------------------------------------------
    def _node_for(self, name):
        parts = name.split(".")
        mod = self
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Node())
            mod = mod._modules[p]
        return mod, parts[-1]

    def _apply(self, fn, recurse=True):
        # Parameters alias flat device buffers: only same-device no-op moves are legal.
        probe = fn(self.flat_params)
        if probe.device != self.flat_params.device or probe.dtype != self.flat_params.dtype:
            raise RuntimeError("ubpl_amd StackedHourglass lives on its GPU in float32 (flat buffers); "
                               "moving it to %s/%s is not supported" % (probe.device, probe.dtype))
        return self

    def P(self, name):
        s, n, shp = self._offs[name]
        return self.flat_params[s:s + n].view(shp)

    def G(self, name):
        s, n, shp = self._offs[name]
        return self.flat_grads[s:s + n].view(shp)

    def stats(self, bn):
        s, c = self._sidx[bn]
        return self.flat_stats[s:s + c], self.flat_stats[s + c:s + 2 * c]

    def set_conv_precision(self, name):
        """Conv arithmetic (kernels.CONV_PRECISIONS; None = $UBPL_CONV_PRECISION or the default):
        'f32'    every conv on the exact-f32 MFMA (conv_f32_fwd.hip, conv1x1_dma.hip, conv_f32_wgrad.hip);
        '6xbf16' the 3x3 convs (forward and data gradient) on split-bf16 MFMA with
                 3 bf16 pieces per operand over pre-split activations (conv_psa.hip, conv_psah.hip
                 PSA path, error at the f32 path's level), the 1x1 convs whose
                 planes fill the chip on the same arithmetic with the activations
                 split while they are staged, the rest f32;
        '2xfp16' the forward convs as '6xbf16' places them, on 2 fp16 pieces of the
                 power-of-two-scaled operands (3 MFMA products instead of 6, operands
                 to 2^-22); the 3x3 data and weight gradients too, their dy scaled
                 by the power of two the BN backward's bound of it picks
                 (UBPL_FP16_BWD3=0: on 6xbf16); the 1x1 gradients on 6xbf16;
        'bf16'   every conv with 16-channel contraction groups (3x3 and 1x1, forward
                 and data gradient) with ONE piece per operand = bf16 operands, f32
                 accumulation (BASELINE config 5's throughput path): 1x1 convs whose
                 plane fills the chip on the split-on-load kernel (no pre-split pass),
                 the rest on the PSA kernels; weight gradients on the PSA (3x3) and
                 split-on-load (1x1, 128-multiple channels) kernels, the other 1x1
                 weight gradients exact f32.
        The stem (7x7, stride 2, 3 input channels) runs in f32 except on the
        6xbf16 space-to-depth path."""
        self.conv_pieces = Kn.conv_precision_pieces(name)          # the forward's
        self.bwd_pieces = Kn.backward_pieces(self.conv_pieces)      # the gradients'
        # the 3x3 convs' gradients (data and weight) on the forward's 2xfp16 too
        self.bwd3_pieces = 2 if self.conv_pieces == 2 and _FP16_BWD3 else self.bwd_pieces
        self._build_weight_tables()

    def _build_weight_tables(self):
        self._wsp, self._wlay = build_weight_tables(self._table, self._offs, self._device, self.conv_pieces,
                                                    self.bwd_pieces, self.bwd3_pieces)
        self._wset = _WeightSet(self._offs, self.flat_params, self._wsp, self._wlay, self.conv_pieces)

    def relayout_weights(self, mode):
        self._wset.relayout(mode)

    def W(self, mode, name):
        return self._wset.W(mode, name)

    def SW(self, mode, name):
        """Split weights of a conv (None when it is not on the split path)."""
        return self._wset.SW(mode, name)

    def _coef_index(self):
        """({BN name: (offset, C)}, total channels) of a forward's coefficient buffer: per BN
        4*C floats, scale|shift|mean|invstd."""
        cidx, o = {}, 0
        for b in self._bn_names:
            c = self._offs[b + ".weight"][1]
            cidx[b] = (o, c)
            o += 4 * c
        return cidx, o // 4

    def freeze(self):
        """A private, frozen copy of what an eval forward reads of the weights (see
        _WeightSet): filled by its refresh(), read by forward_frozen.  Nothing of the
        model is touched, then or later."""
        own = self._wset
        keys = [("rest", 0), ("rest", 1)] if own.pieces else [0, 1]
        wsp = {0: [[tbl, plane, idx, torch.empty_like(buf), pieces] for tbl, plane, idx, buf, pieces in own.wsp[0]],
               1: []}          # (the data-gradient tables are no part of a frozen set)
        wlay = {k: (own.wlay[k][0], torch.empty_like(own.wlay[k][1])) + own.wlay[k][2:] for k in keys}
        ws = _WeightSet(self._offs, torch.empty_like(self.flat_params), wsp, wlay, own.pieces)
        cidx, C = self._coef_index()
        ws.coef = torch.zeros(4 * C, device=self._device)
        rows = []
        for b in self._bn_names:
            s, c = self._sidx[b]
            rows.append((self._offs[b + ".weight"][0], self._offs[b + ".bias"][0], s, s + c, cidx[b][0], c))
        ws.bn_table = Kn.bn_coeff_table(rows, self.n_total, self.flat_stats.numel(), 4 * C).to(self._device)
        if own.pieces in (1, 2, 3):
            cout, np_ = self._offs["pre.0.conv.weight"][2][0], Kn.backward_pieces(own.pieces)
            ws.stem = Kn.SplitWeights(torch.empty(np_ * cout * 256, dtype=torch.int16, device=self._device),
                                      cout * 256, 0, (cout, 16, 16), np_)
        ws.frozen, ws.source = True, self
        ws.refresh()
        return ws

    def forward_frozen(self, imgs, wset):
        """The eval forward from a frozen weight set (freeze()): preds [B,S,K,R,R] alone (no
        feature projection); no weight re-layout, stem-weight split or coefficient launch."""
        _lib.require_gpu(imgs)
        if imgs.dtype != torch.float32 or not imgs.is_contiguous():
            raise TypeError("imgs must be contiguous float32")
        if not getattr(wset, "frozen", False) or wset.source is not self:
            raise ValueError("ubpl_amd: forward_frozen takes a weight set of this model's freeze()")
        with torch.no_grad():
            return self._forward_impl(imgs, save=False, wset=wset)[0]

    def alt_grad_buffer(self):
        """Second gradient buffer for a backward pass that runs concurrently with
        another of the same network (train.py: a student's second view on its
        idle teacher's stream); merge_alt_grads adds it into flat_grads."""
        if getattr(self, "_alt_grads", None) is None:
            self._alt_grads = torch.zeros_like(self.flat_grads)
            self._alt_pending = []
        return self._alt_grads

    def merge_alt_grads(self, release=True):
        """flat_grads += the concurrent pass's gradients (on the current stream,
        after it has joined that pass's stream).  release=False keeps the
        tensors the backward streams read (upstream gradients, the concurrent
        pass's saved activations) alive: a caller merging on a side stream
        releases them with release_backward_refs() after the main stream has
        joined it — freed earlier, the caching allocator could hand their
        blocks to main while those kernels still read them."""
        if getattr(self, "_alt_pending", None):
            # (the library's add: no packed-FP32 instructions, see csrc/Makefile NOPK; this may run on a
            # side stream beside other networks' backward)
            Kn.add(self.flat_grads, self._alt_grads, out=self.flat_grads)
            self._alt_grads.zero_()
            self._alt_done = self._alt_pending
            self._alt_pending = []
        if release:
            self.release_backward_refs()

    def release_backward_refs(self):
        self._alt_done = []
        self._grad_keep = []

    def live_params(self):
        return self.flat_params[:self.n_live]

    def live_grads(self):
        return self.flat_grads[:self.n_live]

    def attach_grad_views(self):
        """Make every parameter's .grad alias flat_grads (for torch optimizers)."""
        for name, p in self.named_parameters():
            if self._offs[name][0] < self.n_live:      # dead skip_layer params keep grad None
                p.grad = self.G(name)
        self._grad_views_attached = True

    def zero_grad(self, set_to_none=True):
        self.flat_grads.zero_()
        self.attach_grad_views()

    # -- forward ----------------------------------------------------------
    def forward(self, imgs):
        _lib.require_gpu(imgs)
        if imgs.dtype != torch.float32:
            raise TypeError("imgs must be float32")
        imgs = imgs.contiguous()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if need_grad and not self.training:
            raise RuntimeError("ubpl_amd: backward through eval-mode BatchNorm is not supported")
        if need_grad:
            preds, feats = _HourglassFn.apply(imgs, self._anchor(), self)
        else:
            with torch.no_grad():
                preds, feats, _ = self._forward_impl(imgs, save=False)
        if self.mode == "default":
            return preds
        return preds, feats

    def _anchor(self):
        a = getattr(self, "_anchor_t", None)
        if a is None:
            a = torch.zeros((), device=self.flat_params.device, requires_grad=True)
            self._anchor_t = a
        return a

    def _scratch(self, B, C):
        key = ("part", B)
        if key not in self._ws:
            n = 0
            for c in (64, 128, 256, 512):
                n = max(n, int(_lib.lib().ubpl_bn_part_doubles(B, c)))
            # zeroed once: the arrival counters at its tail reset themselves
            self._ws[key] = torch.zeros(n, dtype=torch.float64, device=self.flat_params.device)
            self._ws[("coef", B)] = torch.empty(3 * 512 + 4, device=self.flat_params.device)
        return self._ws[key]

    def _forward_impl(self, imgs, save, wset=None):
        """wset: a frozen weight set (freeze()) — an eval forward whatever the training
        flag, with no re-layout, no coefficient launches and no feature projection."""
        B = imgs.shape[0]
        dev = imgs.device
        part = self._scratch(B, 64)
        if save:
            self._grad_keep = []     # the last step's upstream gradients (its streams joined since)
        frozen = wset is not None
        train = self.training and not frozen
        ex = _Exec(self, B, dev, part, train=train, save=save, wset=wset)
        if not frozen:
            self.relayout_weights(0)
            self.relayout_weights(1)       # k-major 1x1 weights for conv1x1_forward_kmajor
        if train:
            self._nbt.add_(1)
        elif not frozen:
            ex.eval_coeffs()
        x = ex.stem(imgs)
        x = ex.residual("pre.1", x)
        x1 = x
        if ex.fuse_ok(x1) and ex.fuse == 2:
            x = ex.bn_maxpool(None, x1, "pre.3.bn1")       # (no BatchNorm takes x1 itself)
            ex.give_coef(x, "pre.3.bn1")
        else:
            x = Kn.maxpool2x2(x1)
        ex.save("pre.2", x1)
        x = ex.residual("pre.3", x)
        x = ex.residual("pre.4", x)
        preds, feats = [], []
        for i in range(self.nStack):
            hg = ex.hourglass("hgs.%d.0" % i, 4, x, "features.%d.0.bn1" % i)
            f0 = ex.residual("features.%d.0" % i, hg)
            f = ex.conv_bn_relu("features.%d.1" % i, f0)
            if self.mode != "default" and not frozen:
                feats.append(Kn.avgpool2x2(f) if self.mode == "AvgPool" else Kn.maxpool2x2(f))
            pr = ex.conv("preds.%d.conv" % i, f)
            preds.append(pr)
            if i < self.nStack - 1:
                t = ex.conv("merge_preds.%d.conv.conv" % i, pr, res=x)
                x = ex.conv("merge_features.%d.conv.conv" % i, f, res=t, out=t)
            ex.save("stack.%d" % i, (f, pr))
        P = torch.stack(preds, 1)
        Fs = torch.stack(feats, 1) if feats else None
        return P, Fs, ex

    # -- backward ---------------------------------------------------------
    def _backward_impl(self, ex, dpreds, dfeats):
        ex.backward(dpreds, dfeats)


class _HourglassFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, imgs, anchor, model):
        preds, feats, ex = model._forward_impl(imgs, save=True)
        ctx.ex = ex
        ctx.model = model
        if feats is None:
            feats = preds.new_empty(0)
        return preds, feats

    @staticmethod
    def backward(ctx, dpreds, dfeats):
        model = ctx.model
        ex = ctx.ex
        if ex.bwd_stream is not None:
            # a second view's backward on another (idle) stream, into the
            # alternate gradient buffer; the caller joins that stream and merges
            if dfeats is not None and dfeats.numel() == 0:
                dfeats = None
            s = ex.bwd_stream
            s.wait_stream(torch.cuda.current_stream(s.device))
            with torch.cuda.stream(s):
                model._backward_impl(ex, dpreds, dfeats)
            model._alt_pending.append((ex, dpreds, dfeats))   # alive until the join
            return None, None, None
        # torch optimizers may have reset .grad to None (zero_grad(set_to_none));
        # then the flat buffer is stale and is restarted from zero.
        first = next(iter(model.parameters()))
        if first.grad is None or first.grad.data_ptr() != model.flat_grads.data_ptr() + 4 * model._offs[
                model._table[0][0]][0]:
            model.flat_grads.zero_()
            model.attach_grad_views()
        if dfeats is not None and dfeats.numel() == 0:
            dfeats = None
        # the upstream gradients come from the loss backward on the main stream
        # and are read here on this network's stream; kept alive until the
        # caller has joined that stream (merge_alt_grads), or the caching
        # allocator hands their blocks back to main while these kernels still
        # read them (a race that shows once nothing paces the launches: the
        # captured step)
        model._grad_keep.append((dpreds, dfeats))
        # the saved activations stay with ctx: the reference runs backward(retain_graph=True)
        # once per student and the shared FDL term reaches both networks twice
        model._backward_impl(ctx.ex, dpreds, dfeats)
        return None, None, None


def pose_model(modelType, kpsCount, mode="default", nograd=False):
    """models/pose/pose_model.py:5-13 ('HG<n>' only; LitePose is out of scope)."""
    if "HG" not in modelType:
        raise ValueError("only HG<n> models are on the HIP path (got %r)" % modelType)
    model = StackedHourglass(kpsCount, int(modelType[len("HG"):]), mode)
    if nograd:
        for p in model.parameters():
            p.detach_()
    return model


PoseModel = pose_model


def hg(k, nStack=3, mode="default", nograd=False):
    """models/pose/hourglass.py:102-107."""
    return pose_model("HG%d" % nStack, k, mode, nograd)
