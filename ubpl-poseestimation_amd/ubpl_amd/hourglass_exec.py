"""The stacked hourglass's executor (hourglass.py): one forward pass over the HIP
kernels, the tensors it saves and its backward — one route per conv precision."""
import os

import torch

from . import kernels as Kn

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
# 2xfp16: the 3x3 data / weight gradients on 2xfp16 too (dy scaled by the BN backward's bound of
# it, bn_bwd.hip bwd_stats_kernel BOUND); UBPL_FP16_BWD3=0: on 6xbf16 (with the forward's 6xbf16 image
# kept for the weight gradient)
_FP16_BWD3 = os.environ.get("UBPL_FP16_BWD3", "1") != "0"
# the hourglass max-pool / upsample-add passes folded into the BatchNorm kernels next to them
# (bn_fwd.hip stats_maxpool_kernel, upadd_stats_kernel; bn_bwd.hip bwd_apply_*_kernel<true>).  UBPL_POOL_FUSE=0: the
# separate launches; 1 (default): every fusion whose results are bit-identical to those launches
# (the pooled tensor's own statistics stay a stats_kernel launch); 2: the pooled tensor's
# statistics from the pooling kernel too — one launch less per level, but a new summation order,
# so the step no longer computes bit for bit what the separate launches do.  Training forwards on
# planes Kn.pool_fuse_ok takes only
_POOL_FUSE = {"0": 0, "2": 2}.get(os.environ.get("UBPL_POOL_FUSE", "1"), 1)


class _Exec:
    def __init__(self, model, B, dev, part, train, save, wset=None):
        self.m, self.B, self.dev, self.part, self.train, self.do_save = model, B, dev, part, train, save
        # the weights the forward reads: the model's own set, or a frozen one (its re-layouts,
        # stem split and eval coefficients made by its refresh(), none of them here)
        self.ws = model._wset if wset is None else wset
        # backward on another stream into the alternate gradient buffer (train.py sets
        # model._bwd_stream around a student's second-view forward)
        self.bwd_stream = getattr(model, "_bwd_stream", None) if save else None
        self.gbuf = model.alt_grad_buffer() if self.bwd_stream is not None else model.flat_grads
        if self.bwd_stream is not None:
            key = ("alt", B)
            if key not in model._ws:
                model._ws[key] = (torch.zeros_like(part), torch.empty(3 * 512 + 4, device=dev))
            self.bpart, self.bcoef = model._ws[key]
        else:
            self.bpart, self.bcoef = part, None
        self.saved = {}
        self.saved_split = {}
        self._rc = None     # (tensor, BN name): its producer filled that BN's coefficients (the fused pool kernels)
        self.fuse = _POOL_FUSE if train else 0      # (0 / 1 / 2: see _POOL_FUSE)
        self.cidx, C = model._coef_index()
        # per BN: scale|shift|mean|invstd
        self.coef = self.ws.coef if self.ws.frozen else torch.empty(4 * C, device=dev)

    # ---- bookkeeping
    def save(self, key, val):
        if self.do_save:
            self.saved[key] = val

    def give_coef(self, y, bn):
        """y's producer computed BatchNorm bn's statistics of it (coefficients and running
        statistics written): the residual that takes y next launches nothing for its bn1."""
        self._rc = (y, bn)

    def take_coef(self, x, bn):
        rc, self._rc = self._rc, None
        return rc is not None and rc[0] is x and rc[1] == bn

    def fuse_ok(self, x):
        """x [B,C,H,W] takes the fused pool / upsample-add + BatchNorm kernels (training forward)."""
        return self.fuse > 0 and Kn.pool_fuse_ok(x.shape[2], x.shape[3], x.shape[1], x)

    def _bn_args(self, name):
        sc, sh, mu, istd = self.bnc(name)
        rm, rv = self.m.stats(name)
        return self.ws.P(name + ".weight"), self.ws.P(name + ".bias"), rm, rv, mu, istd, sc, sh

    def bn_maxpool(self, bn, x, pbn):
        """bn's statistics of x (None: no BatchNorm on x), maxpool2x2(x) and pbn's statistics
        of the pooled tensor in one launch (the caller hands them over: give_coef)."""
        return Kn.bn_forward_stats_maxpool(x, None if bn is None else self._bn_args(bn),
                                           None if pbn is None else self._bn_args(pbn), BN_EPS, BN_MOMENTUM, self.part)

    def bnc(self, bn):
        o, c = self.cidx[bn]
        v = self.coef[o:o + 4 * c]
        return v[:c], v[c:2 * c], v[2 * c:3 * c], v[3 * c:]

    def eval_coeffs(self):
        for b in self.m._bn_names:
            sc, sh, _, _ = self.bnc(b)
            rm, rv = self.m.stats(b)
            Kn.bn_eval_coeffs(self.ws.P(b + ".weight"), self.ws.P(b + ".bias"), rm, rv, BN_EPS, sc, sh)

    def bn(self, name, x):
        """Train: batch statistics (+ running-stat update) by a pass over x; eval: precomputed."""
        sc, sh, mu, istd = self.bnc(name)
        if self.train:
            rm, rv = self.m.stats(name)
            g, b = self.ws.P(name + ".weight"), self.ws.P(name + ".bias")
            Kn.bn_forward_stats(x, g, b, BN_EPS, BN_MOMENTUM, rm, rv, self.part, mu, istd, sc, sh)
        return sc, sh

    def conv(self, name, x, stride=1, pro=None, res=None, out=None):
        w = self.ws.P(name + ".weight")
        b = self.ws.P(name + ".bias")
        ps, ph = (None, None) if pro is None else pro
        ws = self.ws.SW(0, name + ".weight") if stride == 1 else None
        if ws is not None and ws.npieces in (1, 2, 3) and ws.shape[1] == 1:
            if Kn.conv1x1_split_load_ok(x, ws, small=self.ws.pieces == 2):
                return Kn.conv1x1_forward_split_load(x, ws, b, ps, ph, res=res, out=out)
            if ws.npieces in (2, 3):
                ws = None                                # small plane: the f32 1x1 kernel (bf16: the PSA kernel)
        if ws is not None:                               # (npieces 1, 2 or 3: every precision SW knows)
            keep = self.do_save and ws.shape[1] == 9
            if ws.npieces == 2 and keep and self.m.bwd3_pieces == 3:
                # 2xfp16 forward, 6xbf16 gradients: the conv's fp16 image and, from the same
                # read, the 6xbf16 one its weight gradient takes
                xs, xs3 = Kn.split_activation(x, 2, 1, ps, ph, with3=True)
                self.saved_split[name] = xs3
            else:
                xs = Kn.split_activation(x, ws.npieces, (ws.shape[1] == 9) * 1, ps, ph)
                if keep:
                    self.saved_split[name] = xs      # the 3x3 weight gradient's B operand
            return Kn.conv2d_forward_psa(xs, ws, b, res=res, out=out)
        if w.shape[2] == 1 and stride == 1 and Kn.conv1x1_kmajor_ok(x, w.shape[0]):
            return Kn.conv1x1_forward_kmajor(x, self.ws.W(1, name + ".weight"), b, ps, ph, res=res, out=out)
        wt = self.ws.W(0, name + ".weight") if w.shape[2] > 1 else None
        return Kn.conv2d_forward(x, w, b, stride, ps, ph, res=res, out=out, w_tap=wt)

    # ---- layers
    def stem(self, imgs):
        if self.ws.pieces in (1, 2, 3) and Kn.stem_s2d_ok(imgs):
            # 7x7/s2 as a 4x4 stride-1 conv over the space-to-depth image, on the split path
            # (6xbf16, also under 2xfp16: the image is its weight gradient's operand), or on
            # bf16 operands (the "bf16" precision)
            np_ = Kn.backward_pieces(self.ws.pieces)
            ws = self.ws.stem_split(np_)
            xs = Kn.stem_s2d_split(imgs, 2, np_)
            y0 = Kn.conv2d_forward_psa(xs, ws, self.ws.P("pre.0.conv.bias"))
            if self.do_save:
                self.saved_split["pre.0.conv"] = xs      # the weight gradient's B operand
        else:
            y0 = self.conv("pre.0.conv", imgs, stride=2)
        sc, sh = self.bn("pre.0.bn", y0)
        x0 = Kn.bn_apply(y0, sc, sh, relu=1)
        self.save("pre.0", (imgs, y0))
        return x0

    def conv_bn_relu(self, p, x):
        y = self.conv(p + ".conv", x)
        sc, sh = self.bn(p + ".bn", y)
        f = Kn.bn_apply(y, sc, sh, relu=1)
        self.save(p, (x, y))
        return f

    def residual(self, p, x):
        """models/base/layers.py:69-84 (pre-activation bottleneck)."""
        cin = x.shape[1]
        cout = self.m._offs[p + ".conv3.conv.weight"][2][0]
        c1 = self.bnc(p + ".bn1")[:2] if self.take_coef(x, p + ".bn1") else self.bn(p + ".bn1", x)
        t1 = self.conv(p + ".conv1.conv", x, pro=c1)
        c2 = self.bn(p + ".bn2", t1)
        t2 = self.conv(p + ".conv2.conv", t1, pro=c2)
        c3 = self.bn(p + ".bn3", t2)
        if cin != cout:
            r = self.conv(p + ".skip_layer.conv", x)
            out = self.conv(p + ".conv3.conv", t2, pro=c3, res=r, out=r)
        else:
            out = self.conv(p + ".conv3.conv", t2, pro=c3, res=x)
        self.save(p, (x, t1, t2))
        return out

    def hourglass(self, p, n, x, consumer=None):
        """models/base/layers.py:104-111.  consumer: the BatchNorm that takes the result
        (the bn1 of the residual after it), for the fused upsample-add."""
        if self.fuse_ok(x):
            # up1.bn1's statistics launch also pools x
            # (fuse == 2 only: and takes low1.bn1's statistics of the pooled tensor)
            pl = self.bn_maxpool(p + ".up1.bn1", x, p + ".low1.bn1" if self.fuse == 2 else None)
            self.give_coef(x, p + ".up1.bn1")
            up1 = self.residual(p + ".up1", x)
            if self.fuse == 2:
                self.give_coef(pl, p + ".low1.bn1")
        else:
            up1 = self.residual(p + ".up1", x)
            pl = Kn.maxpool2x2(x)
        low1 = self.residual(p + ".low1", pl)
        low2 = self.hourglass(p + ".low2", n - 1, low1, p + ".low3.bn1") if n > 1 else \
            self.residual(p + ".low2", low1)
        low3 = self.residual(p + ".low3", low2)
        self.save(p, x)
        if consumer is not None and self.fuse_ok(up1) and low3.data_ptr() % 8 == 0:
            # the add in place, with the consumer's statistics of the sum
            out = Kn.upsample2x_add_bnstats(up1, low3, self._bn_args(consumer), BN_EPS, BN_MOMENTUM, self.part,
                                            out=up1)
            self.give_coef(out, consumer)
            return out
        return Kn.upsample2x_add(up1, low3, out=up1)

    # ---- backward
    def _coef(self):
        return self.bcoef if self.bcoef is not None else self.m._ws[("coef", self.B)]

    def G(self, name):
        s, n, shp = self.m._offs[name]
        return self.gbuf[s:s + n].view(shp)

    def bn_bwd(self, name, dz, x, relu, add1=None, add2=None, out=None, pool_dy=None):
        """pool_dy: the gradient of maxpool2x2(x), added between add1 and add2."""
        sc, sh, mu, istd = self.bnc(name)
        if pool_dy is not None:
            return Kn.bn_backward_pool(dz, x, self.m.P(name + ".weight"), mu, istd, sc, sh, relu, self.bpart,
                                       self._coef(), self.G(name + ".weight"), self.G(name + ".bias"), add1=add1,
                                       pool_dy=pool_dy, add2=add2, out=out)
        return Kn.bn_backward(dz, x, self.m.P(name + ".weight"), mu, istd, sc, sh, relu, self.bpart, self._coef(),
                              self.G(name + ".weight"), self.G(name + ".bias"), add1=add1, add2=add2, out=out)

    def bn_bwd_split(self, name, dz, x, relu, pieces=None, grads=True):
        """dx as the split operand (pieces: the consumer's; 2 = 2xfp16 with its device-side
        scale); grads=False: the BN's own parameter gradients not accumulated (a second
        pass over the same dz)."""
        sc, sh, mu, istd = self.bnc(name)
        return Kn.bn_backward_split(dz, x, self.m.P(name + ".weight"), mu, istd, sc, sh, relu, self.bpart,
                                    self._coef(), self.G(name + ".weight") if grads else None,
                                    self.G(name + ".bias") if grads else None,
                                    self.m.bwd_pieces if pieces is None else pieces, 1)

    def wgrad(self, name, dy, x, KS, stride=1, pro=None):
        ps, ph = (None, None) if pro is None else pro
        if KS == 1 and self.m.bwd_pieces in (1, 3) and Kn.wgrad1x1_split_load_ok(dy, x):
            Kn.conv2d_wgrad1x1_split_load(dy, x, self.G(name + ".weight"), self.G(name + ".bias"), ps, ph,
                                          accumulate=True, npieces=self.m.bwd_pieces)
            return
        Kn.conv2d_wgrad(dy, x, KS, stride, self.G(name + ".weight"), self.G(name + ".bias"), ps, ph,
                        accumulate=True)

    def dgrad(self, name, dy, res=None, out=None):
        ws = self.m.SW(1, name + ".weight")
        if ws is not None and ws.npieces in (1, 3) and ws.shape[1] == 1:
            if Kn.conv1x1_split_load_ok(dy, ws, small=self.m.conv_pieces == 2):
                return Kn.conv1x1_forward_split_load(dy, ws, None, res=res, out=out)
            if ws.npieces == 3:
                ws = None
        if ws is not None:   # (npieces 1 or 3: the 2xfp16 3x3 data gradients run in residual_bwd)
            ys = Kn.split_activation(dy, ws.npieces, (ws.shape[1] == 9) * 1)
            return Kn.conv2d_forward_psa(ys, ws, None, res=res, out=out)
        w = self.m.P(name + ".weight")
        if w.shape[2] == 1 and Kn.conv1x1_kmajor_ok(dy, w.shape[1]):
            return Kn.conv1x1_forward_kmajor(dy, w, None, res=res, out=out)     # [Cout][Cin] = k-major
        return Kn.conv2d_dgrad(dy, None, res=res, out=out, wt=self.m.W(1, name + ".weight"))

    def residual_bwd(self, p, dout, pool_dy=None, add2=None):
        """pool_dy / add2: folded into the final bn1 apply (the input was also max-pooled;
        a second gradient of the input), see bn_bwd."""
        x, t1, t2 = self.saved.get(p)
        cin = x.shape[1]
        cout = dout.shape[1]
        c1 = self.bnc(p + ".bn1")[:2]
        c2 = self.bnc(p + ".bn2")[:2]
        c3 = self.bnc(p + ".bn3")[:2]
        self.wgrad(p + ".conv3.conv", dout, t2, 1, pro=c3)
        d = self.dgrad(p + ".conv3.conv", dout)                       # d relu(bn3(t2))
        ws = self.m.SW(1, p + ".conv2.conv.weight")
        xs = self.saved_split.get(p + ".conv2.conv")
        split_wgrad = (ws is not None and ws.npieces in (1, 2, 3) and xs is not None and t2.shape[1] % 64 == 0
                       and xs.C % 64 == 0 and t2.shape[3] % 16 == 0 and xs.npieces == ws.npieces)
        if split_wgrad:
            # d t2 only as the split operand both conv2 gradients read
            ys = self.bn_bwd_split(p + ".bn3", d, t2, relu=1, pieces=ws.npieces)
            Kn.conv2d_wgrad3_psa(ys, xs, self.G(p + ".conv2.conv.weight"), self.G(p + ".conv2.conv.bias"))
            d = Kn.conv2d_forward_psa(ys, ws, None)                   # d relu(bn2(t1))
        elif ws is not None and ws.npieces in (1, 2, 3):
            ys = None
            if ws.npieces == 2:
                # the data gradient's 2xfp16 operand with its bound-derived scale, from a second
                # statistics pass over the same dz (the BN's parameter gradients accumulate once, below)
                ys = self.bn_bwd_split(p + ".bn3", d, t2, relu=1, pieces=2, grads=False)
            d = self.bn_bwd(p + ".bn3", d, t2, relu=1)                # d t2
            self.wgrad(p + ".conv2.conv", d, t1, 3, pro=c2)
            d = Kn.conv2d_forward_psa(ys if ys is not None else Kn.split_activation(d, ws.npieces, 1), ws, None)
        else:
            d = self.bn_bwd(p + ".bn3", d, t2, relu=1)                # d t2
            self.wgrad(p + ".conv2.conv", d, t1, 3, pro=c2)
            d = self.dgrad(p + ".conv2.conv", d)                       # d relu(bn2(t1))
        d = self.bn_bwd(p + ".bn2", d, t1, relu=1)                    # d t1
        self.wgrad(p + ".conv1.conv", d, x, 1, pro=c1)
        d = self.dgrad(p + ".conv1.conv", d)                          # d relu(bn1(x))
        if cin != cout:
            self.wgrad(p + ".skip_layer.conv", dout, x, 1)
            ds = self.dgrad(p + ".skip_layer.conv", dout)
            return self.bn_bwd(p + ".bn1", d, x, relu=1, add1=ds, pool_dy=pool_dy, add2=add2)
        return self.bn_bwd(p + ".bn1", d, x, relu=1, add1=dout, pool_dy=pool_dy, add2=add2)

    def hourglass_bwd(self, p, n, dout, add2=None):
        """add2: a second gradient of the hourglass input (the next stack's), added last."""
        x = self.saved.get(p)
        B, C, H, W = dout.shape
        dlow3 = torch.empty((B, C, H // 2, W // 2), device=self.dev)
        Kn.upsample2x_add_backward(dout, dlow3, accumulate=False)
        dlow2 = self.residual_bwd(p + ".low3", dlow3)
        dlow1 = self.hourglass_bwd(p + ".low2", n - 1, dlow2) if n > 1 else self.residual_bwd(p + ".low2", dlow2)
        dpl = self.residual_bwd(p + ".low1", dlow1)
        if _POOL_FUSE and Kn.pool_fuse_ok(x.shape[2], x.shape[3], x.shape[1], x, dout, dpl, add2):
            # the pool's gradient and add2 inside up1.bn1's backward apply
            return self.residual_bwd(p + ".up1", dout, pool_dy=dpl, add2=add2)
        dx = self.residual_bwd(p + ".up1", dout)
        Kn.maxpool2x2_backward(x, dpl, dx, accumulate=True)
        if add2 is not None:
            dx = Kn.add(dx, add2, out=dx)
        return dx

    def backward(self, dpreds, dfeats):
        m = self.m
        S = m.nStack
        # the data-gradient weights (mode 1) were laid out by the forward
        # (_forward_impl) and the weights are unchanged since: no re-layout
        # here, which would rewrite them while a concurrent pass of the same
        # network (a second view on the teacher's stream) reads them
        dpreds = dpreds.contiguous()
        if dfeats is not None:
            dfeats = dfeats.contiguous()
        dxn = None                                       # grad of the x entering stack i+1
        for i in reversed(range(S)):
            f, pr = self.saved.get("stack.%d" % i)
            dpi = dpreds[:, i].contiguous()
            if i < S - 1:
                nmf, nmp = "merge_features.%d.conv.conv" % i, "merge_preds.%d.conv.conv" % i
                self.wgrad(nmf, dxn, f, 1)
                self.wgrad(nmp, dxn, pr, 1)
                dpi = self.dgrad(nmp, dxn, res=dpi, out=dpi)
            npd = "preds.%d.conv" % i
            self.wgrad(npd, dpi, f, 1)
            df = self.dgrad(npd, dpi)
            if i < S - 1:
                df = self.dgrad(nmf, dxn, res=df, out=df)
            if dfeats is not None:
                dfi = dfeats[:, i].contiguous()
                if m.mode == "AvgPool":
                    Kn.avgpool2x2_backward(dfi, df, accumulate=True)
                else:
                    Kn.maxpool2x2_backward(f, dfi, df, accumulate=True)
            f0, yf = self.saved.get("features.%d.1" % i)
            d = self.bn_bwd("features.%d.1.bn" % i, df, yf, relu=1)
            self.wgrad("features.%d.1.conv" % i, d, f0, 1)
            d = self.dgrad("features.%d.1.conv" % i, d)
            d = self.residual_bwd("features.%d.0" % i, d)
            dxn = self.hourglass_bwd("hgs.%d.0" % i, 4, d, add2=dxn)
        d = self.residual_bwd("pre.4", dxn)
        d = self.residual_bwd("pre.3", d)
        x1 = self.saved.get("pre.2")
        dx1 = torch.empty_like(x1)                       # (even H, W: every element written)
        Kn.maxpool2x2_backward(x1, d, dx1, accumulate=False)
        d = self.residual_bwd("pre.1", dx1)
        imgs, y0 = self.saved.get("pre.0")
        xs = self.saved_split.get("pre.0.conv")
        w0 = m.P("pre.0.conv.weight")
        if xs is not None and m.bwd_pieces in (1, 3) and d.shape[1] % 64 == 0 and d.shape[3] % 16 == 0:
            # dy of the stem only as the split operand of its weight gradient (the input
            # image takes no gradient): the space-to-depth 4x4 weight gradient, mapped to 7x7
            ys = self.bn_bwd_split("pre.0.bn", d, y0, relu=1)
            if Kn.wgrad_stem_psa_ok(ys, xs, w0):
                Kn.conv2d_wgrad_stem_psa(ys, xs, self.G("pre.0.conv.weight"), self.G("pre.0.conv.bias"))
                return
            raise RuntimeError("ubpl_amd: stem weight gradient operands %s / %s" % (
                (ys.B, ys.C, ys.H, ys.W, ys.pad), (xs.B, xs.C, xs.H, xs.W, xs.pad)))
        d = self.bn_bwd("pre.0.bn", d, y0, relu=1)
        self.wgrad("pre.0.conv", d, imgs, 7, stride=2)
