"""The conv precisions and the split operands they run on (SplitWeights, SplitAct): what the
conv and the BatchNorm wrappers both need, so neither imports the other."""
import os

# Conv arithmetic: "f32" = exact-f32 MFMA (v_mfma_f32_32x32x2_f32); "6xbf16" =
# split-bf16 MFMA with 3 bf16 pieces per f32 operand (6 piece products, f32
# accumulation: exact operands); "2xfp16" = the forward convs (students' and
# teachers') with 2 fp16 pieces per operand of the power-of-two-scaled value (3
# piece products on the fp16 MFMA, operands to 2^-22: split_common.h / common.h
# split2), the backward (data and weight gradients, whose operands have no
# known range) on 6xbf16; "bf16" = one piece, i.e. both operands rounded to bf16
# (RNE) with f32 accumulation — the throughput precision of BASELINE config 5
# (8 stacks, 384x384), not parity-grade.  Value = the forward's pieces (0 for f32).
CONV_PRECISIONS = {"f32": 0, "bf16": 1, "2xfp16": 2, "6xbf16": 3}
# (round 6: 2xfp16 the default — every network-level parity test green on it, the step 17 % faster)
DEFAULT_CONV_PRECISION = "2xfp16"


def backward_pieces(pieces):
    """Pieces of the data / weight gradients' split operands for a precision's
    forward pieces (2xfp16: the backward runs on 6xbf16)."""
    return 3 if pieces == 2 else pieces


def conv_precision_name(name=None):
    return name or os.environ.get("UBPL_CONV_PRECISION", DEFAULT_CONV_PRECISION)


def conv_precision_pieces(name=None):
    """Pieces for a precision name (default: $UBPL_CONV_PRECISION or DEFAULT_CONV_PRECISION)."""
    name = conv_precision_name(name)
    if name not in CONV_PRECISIONS:
        raise ValueError("conv precision %r not in %s" % (name, sorted(CONV_PRECISIONS)))
    return CONV_PRECISIONS[name]


class SplitWeights:
    """One conv's weights as `npieces` bf16 planes (conv_weights_split.hip): a view into
    a shared buffer `buf` (int16, planes `plane` elements apart) at element
    offset `off`; shape = (rows, KS*KS, cols) of the GEMM A operand."""

    __slots__ = ("buf", "plane", "off", "shape", "npieces")

    def __init__(self, buf, plane, off, shape, npieces):
        self.buf, self.plane, self.off, self.shape, self.npieces = buf, plane, off, shape, npieces

    def ptr(self):
        """The planes' base as a tensor view at element offset `off`."""
        return self.buf[self.off:]


class SplitAct:
    """Pre-split activations (conv_psa.hip PSA layout): `npieces` 16-bit planes of
    [B][C/16][H+2pad][W+2pad][16] in an int16 buffer, planes `plane` elements apart
    (3: bf16 pieces; 2: fp16 pieces of v * 32, the 2xfp16 path; 1: bf16(v))."""

    __slots__ = ("buf", "plane", "B", "C", "H", "W", "pad", "npieces", "scale")

    def __init__(self, buf, plane, B, C, H, W, pad, npieces, scale=None):
        self.buf, self.plane, self.B, self.C, self.H, self.W = buf, plane, B, C, H, W
        self.pad, self.npieces = pad, npieces
        # 2xfp16 images whose power-of-two scale lives on the device (a data gradient's: a
        # one-float tensor); None: the fixed activation scale (32) or no scale
        self.scale = scale
