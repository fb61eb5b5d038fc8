"""The stacked hourglass's parameters (hourglass.py): the table in the reference's
registration order, its default initialisation, the structural module nodes, the
split / re-layout weight tables of a conv precision and the weight set a forward reads."""
import math

import torch
from torch import nn

from . import kernels as Kn
from .hourglass_exec import BN_EPS


# ---------------------------------------------------------------------------
# Parameter table in the reference's registration order
# ---------------------------------------------------------------------------
def build_table(k, nstack):
    """[(name, shape, kind, live)] kind in {'cw','cb','bw','bb'}; live=False for the
    skip_layer of Residual(c, c) (constructed, never used: models/base/layers.py:63-67)."""
    tab = []

    def conv(p, cin, cout, ks, live=True):
        tab.append((p + ".weight", (cout, cin, ks, ks), "cw", live))
        tab.append((p + ".bias", (cout,), "cb", live))

    def bn(p, c):
        tab.append((p + ".weight", (c,), "bw", True))
        tab.append((p + ".bias", (c,), "bb", True))

    def residual(p, cin, cout):
        half = cout // 2
        bn(p + ".bn1", cin)
        conv(p + ".conv1.conv", cin, half, 1)
        bn(p + ".bn2", half)
        conv(p + ".conv2.conv", half, half, 3)
        bn(p + ".bn3", half)
        conv(p + ".conv3.conv", half, cout, 1)
        conv(p + ".skip_layer.conv", cin, cout, 1, live=cin != cout)

    def hourglass(p, n, f):
        residual(p + ".up1", f, f)
        residual(p + ".low1", f, f)
        if n > 1:
            hourglass(p + ".low2", n - 1, f)
        else:
            residual(p + ".low2", f, f)
        residual(p + ".low3", f, f)

    conv("pre.0.conv", 3, 64, 7)
    bn("pre.0.bn", 64)
    residual("pre.1", 64, 128)
    residual("pre.3", 128, 128)
    residual("pre.4", 128, 256)
    for i in range(nstack):
        hourglass("hgs.%d.0" % i, 4, 256)
    for i in range(nstack):
        residual("features.%d.0" % i, 256, 256)
        conv("features.%d.1.conv" % i, 256, 256, 1)
        bn("features.%d.1.bn" % i, 256)
    for i in range(nstack):
        conv("preds.%d.conv" % i, 256, k, 1)
    for i in range(nstack - 1):
        conv("merge_features.%d.conv.conv" % i, 256, 256, 1)
    for i in range(nstack - 1):
        conv("merge_preds.%d.conv.conv" % i, k, 256, 1)
    return tab


def _default_init(tab):
    """nn.Conv2d.reset_parameters / BatchNorm2d defaults, consuming the CPU RNG in
    registration order exactly like the reference constructor."""
    vals = []
    last_w = None
    for name, shape, kind, _ in tab:
        t = torch.empty(shape)
        if kind == "cw":
            nn.init.kaiming_uniform_(t, a=math.sqrt(5))
            last_w = t
        elif kind == "cb":
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(last_w)
            bound = 1 / math.sqrt(fan_in) if fan_in > 0 else 0
            nn.init.uniform_(t, -bound, bound)
        elif kind == "bw":
            t.fill_(1.0)
        else:
            t.zero_()
        vals.append(t)
    return vals


class _Node(nn.Module):
    """Container mirroring one module of the reference tree (params/buffers only)."""

    def forward(self, *a):  # pragma: no cover - never called
        raise RuntimeError("structural node")


STEM = "pre.0.conv.weight"


def build_weight_tables(table, offs, device, conv_pieces, bwd_pieces, bwd3_pieces):
    """(wsp, wlay) of a conv precision.  Split path (wsp[mode]): the convs the precision
    puts there whose contraction runs over 16-channel groups (Cin for the forward, Cout
    for the data gradient); f32 path: wlay[mode] = every conv that needs a re-layout,
    wlay[("rest", mode)] = those of them not on the split path."""
    wsp = {}
    for mode in (0, 1):
        # the pieces of a conv's table: the forward's (mode 0), its gradients' (mode 1: 3x3
        # and 1x1 may differ under 2xfp16) — one batched split launch per piece count
        pieces_of = (lambda ks: conv_pieces) if mode == 0 else \
            (lambda ks: bwd3_pieces if ks == 3 else bwd_pieces)
        tables = {}
        for name, shape, kind, live in table:
            if kind != "cw" or not live or name == STEM:
                continue
            pieces = pieces_of(shape[2])
            if not pieces or shape[1 if mode == 0 else 0] % 16:
                continue
            # 6xbf16 / 2xfp16: 3x3 (PSA path) and 1x1 (split on load; outputs of 16 channels
            # and up, the heatmap projection included)
            if pieces in (2, 3) and not (shape[2] == 3 or (shape[2] == 1 and shape[0 if mode == 0 else 1] % 16 == 0)):
                continue
            rows, idx, o = tables.setdefault(pieces, ([], {}, [0]))
            s, n, _ = offs[name]
            T = shape[2] * shape[3]
            rows.append((s, o[0], shape[0], shape[1], T))
            idx[name] = (o[0], (shape[0], T, shape[1]) if mode == 0 else (shape[1], T, shape[0]))
            o[0] += (n + 7) // 8 * 8
        subs = []
        for pieces, (rows, idx, o) in sorted(tables.items()):
            buf = torch.empty(max(pieces, 1) * max(o[0], 8), dtype=torch.int16, device=device)
            subs.append([torch.tensor(rows, dtype=torch.int64).reshape(-1, 5).to(device), max(o[0], 8), idx, buf,
                         pieces])
        wsp[mode] = subs
    wlay = {}
    for mode in (0, 1):
        need = (lambda ks, nm: ks > 1) if mode == 0 else (lambda ks, nm: nm != STEM)
        # (1x1 convs stay in "rest" too: the f32 kernel takes the small planes)
        on_split = set(nm for sub in wsp[mode] for nm in sub[2])
        for key, keep in ((mode, need), (("rest", mode), lambda ks, nm, f=need, sp=on_split:
                                           f(ks, nm) and (ks == 1 or nm not in sp))):
            rows, idx, o = [], {}, 0
            for name, shape, kind, live in table:
                if kind != "cw" or not live or not keep(shape[2], name):
                    continue
                s, n, _ = offs[name]
                rows.append((s, o, shape[0], shape[1], shape[2] * shape[3]))
                T = shape[2] * shape[3]
                idx[name] = (o, (shape[0], T, shape[1]) if mode == 0 else (shape[1], T, shape[0]))
                o += (n + 3) // 4 * 4
            tbl = torch.tensor(rows, dtype=torch.int64).reshape(-1, 5).to(device)
            wlay[key] = (tbl, torch.empty(max(o, 4), device=device), idx, mode)
    return wsp, wlay


class _WeightSet:
    """What a forward reads of a network's weights: the flat parameters (biases, BN
    affine, the weights the f32 1x1 kernel takes as they are), the split tables and
    buffers (`wsp[mode]`, build_weight_tables) and the f32 re-layouts
    (`wlay[key]`), for the conv precision `pieces`.

    The model's own set aliases flat_params and is re-laid out by every forward.  A
    frozen set (StackedHourglass.freeze) owns copies of the forward's part of it — the
    mode-0 split buffers, the f32 re-layouts the forward reads, the stem's
    space-to-depth split weights (`stem`) and one coefficient buffer (`coef`, the
    executor's scale|shift|mean|invstd blocks with scale and shift filled) — all
    written by refresh() alone, in place, so a captured graph that reads them stays
    valid across refreshes."""

    def __init__(self, offs, params, wsp, wlay, pieces):
        self.offs, self.params, self.wsp, self.wlay, self.pieces = offs, params, wsp, wlay, pieces
        self.frozen, self.source = False, None
        self.stem = self.coef = self.bn_table = None

    def P(self, name):
        s, n, shp = self.offs[name]
        return self.params[s:s + n].view(shp)

    def relayout(self, mode):
        if self.pieces:
            for tbl, plane, _, buf, pieces in self.wsp[mode]:
                Kn.conv_weights_split(self.params, buf, plane, tbl, mode, pieces)
            tbl, buf, _, m = self.wlay[("rest", mode)]
            if tbl.shape[0]:
                Kn.conv_weights_relayout(self.params, buf, tbl, m)
            return
        tbl, buf, _, m = self.wlay[mode]
        Kn.conv_weights_relayout(self.params, buf, tbl, m)

    def W(self, mode, name):
        key = ("rest", mode) if self.pieces else mode
        _, buf, idx, _ = self.wlay[key]
        o, shp = idx[name]
        return buf[o:o + shp[0] * shp[1] * shp[2]].view(shp)

    def SW(self, mode, name):
        """Split weights of a conv (None when it is not on the split path)."""
        if not self.pieces:
            return None
        for _, plane, idx, buf, pieces in self.wsp[mode]:
            if name in idx:
                o, shp = idx[name]
                return Kn.SplitWeights(buf, plane, o, shp, pieces)
        return None

    def stem_split(self, npieces):
        """The stem's space-to-depth split weights: a frozen set's own, else split now."""
        if self.stem is not None:
            return self.stem
        return Kn.stem_weight_s2d_split(self.P(STEM), npieces)

    def refresh(self):
        """Frozen sets: take the source model's current parameters and running statistics —
        one copy, the batched split / re-layout launches, the stem split and ONE
        coefficient launch for every BatchNorm."""
        if not self.frozen:
            raise RuntimeError("ubpl_amd: the model's own weight set follows its parameters; only a frozen set "
                               "is refreshed")
        m = self.source
        self.params.copy_(m.flat_params)
        self.relayout(0)
        self.relayout(1)               # (the k-major 1x1 weights; a frozen set has no mode-1 split tables)
        if self.stem is not None:
            Kn.stem_weight_s2d_split(self.P(STEM), self.stem.npieces, out=self.stem)
        Kn.bn_eval_coeffs_table(self.params, m.flat_stats, self.bn_table, BN_EPS, self.coef)
