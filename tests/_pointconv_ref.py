"""fp64 restatements of the conv5 BatchNorm + LeakyReLU passes (csrc/pointconv.hip,
reference models/dgcnn.py:74-78, 100-102) and the buffers the oracle tests hand
to the C ABI. Everything a kernel receives (Z, dout, scale, shift, mean, invstd,
c0, c1) is given data, so each restatement is the kernel's formula evaluated in
float64 from the same fp32 / bf16 inputs:

  y    = a z + b                      LeakyReLU argument; the fp32 fmaf(a, z, b)
                                      is correctly rounded, so its sign is the
                                      sign of the exact value: decisions agree
                                      everywhere, and points with y == 0 (planted
                                      by make_case) take the slope branch
  out  = y > 0 ? y : slope y          (B, C, N)
  d    = dout * (y > 0 ? 1 : slope)   point-major (M, C)
  s1   = sum_rows d,  s2 = sum_rows d (z - mean) invstd
  dZ   = a d + c0 + c1 z

Tolerances come from the arithmetic, not from runs (u = 2^-24):
  fp32 single-fma outputs   2 u |ref|
  dZ                        4 u (|a d| + |c1 z| + |c0|)
  bf16 outputs              the fp32 bound + 2^-8 |ref|
  column sums               32 u sum|term| (a serial sum plus a shuffle tree is at
                            most ~16 roundings deep, the term itself carries 3)
"""
import torch

U = 2.0 ** -24
SENT = 12288.0          # exactly representable in bf16: untouched output stays bit-equal
NS = (3, 130, 257, 384)
CS = (4, 68, 70, 96, 128)
BS = (1, 3)
SLOPES = (0.2, 0.0)


def f32_value(x):
    """The float32 nearest to the Python float x, as a Python float (what a
    kernel receives for a ``float`` argument)."""
    return float(torch.tensor(x, dtype=torch.float32))


class Case:
    pass


def make_case(dev, B, N, C, seed):
    """Given data of one (B, N, C): scale of both signs, shift small against
    a z so that about half of a z + b falls on each side of zero, channel 1 (or
    0) with shift 0 and z = 0 at every 7th point (exact zeros of a z + b, where
    ``>`` and ``>=`` differ), random dout. ``Zg`` / ``Zbg`` carry one NaN guard
    row after the last point: a kernel that reads past row M poisons its output."""
    g = torch.Generator().manual_seed(seed)
    M = B * N
    c = Case()
    c.B, c.N, c.C, c.M = B, N, C, M
    Z = torch.randn(M, C, generator=g)
    scale = torch.randn(C, generator=g)
    scale[0] = scale[0].abs() + 0.1
    scale[C - 1] = -scale[C - 1].abs() - 0.1
    shift = 0.3 * torch.randn(C, generator=g)
    zc = 1 if C > 1 else 0
    shift[zc] = 0.0
    Z[::7, zc] = 0.0
    Zg = torch.full((M + 1, C), float("nan"))
    Zg[:M] = Z
    c.Zg = Zg.to(dev)
    c.Z = c.Zg[:M]
    c.Zbg = c.Zg.bfloat16()
    c.Zb = c.Zbg[:M]
    c.dout = torch.randn(B, C, N, generator=g).to(dev)
    c.dz_in = torch.randn(M, C, generator=g).to(dev)
    c.scale = scale.to(dev)
    c.shift = shift.to(dev)
    c.mean = (0.1 * torch.randn(C, generator=g)).to(dev)
    c.invstd = (torch.rand(C, generator=g) + 0.5).to(dev)
    c.c0 = (0.1 * torch.randn(C, generator=g)).to(dev)
    c.c1 = (0.1 * torch.randn(C, generator=g)).to(dev)
    return c


def guarded(rows, cols, dev, dtype=torch.float32):
    """(buffer of rows + 1 guard row, all SENT; view of the rows)."""
    full = torch.full((rows + 1, cols), SENT, dtype=dtype, device=dev)
    return full, full[:rows]


def guard_intact(full):
    return bool((full[-1].float() == SENT).all())


def to_mc(t, B, N, C):
    """(B, C, N) -> point-major (M, C)"""
    return t.permute(0, 2, 1).reshape(B * N, C)


def to_bcn(t, B, N, C):
    """point-major (M, C) -> (B, C, N)"""
    return t.view(B, N, C).permute(0, 2, 1)


class Ref:
    """The restatement for one case, one Z (fp32 or its bf16 twin), one slope."""

    def __init__(self, c, Z, slope):
        sl = f32_value(slope)
        B, N, C = c.B, c.N, c.C
        z = Z.double()
        a, b = c.scale.double(), c.shift.double()
        y = a * z + b                       # a z is exact in fp64, the sum rounds once: sign(y) is exact
        self.pos = y > 0
        self.out = to_bcn(torch.where(self.pos, y, y * sl), B, N, C)
        self.d = to_mc(c.dout.double(), B, N, C) * torch.where(self.pos, 1.0, sl)
        zhat = (z - c.mean.double()) * c.invstd.double()
        self.s1, self.s1_abs = self.d.sum(0), self.d.abs().sum(0)
        t2 = self.d * zhat
        self.s2, self.s2_abs = t2.sum(0), t2.abs().sum(0)
        self.z, self.a = z, a
        self.c = c

    def dZ(self, d):
        """(dZ, its magnitude sum) for the point-major d given (fp64)."""
        c = self.c
        t0, t1, t2 = self.a * d, c.c1.double() * self.z, c.c0.double().expand_as(self.z)
        return t0 + t1 + t2, t0.abs() + t1.abs() + t2.abs()


def within(got, ref, bound):
    """every element of got within bound of ref (NaN or a left-over sentinel fails)"""
    return bool(((got.double() - ref).abs() <= bound).all())


def worst(got, ref, bound):
    """largest error / bound over the elements (for the assertion message)"""
    r = (got.double() - ref).abs() / bound.clamp_min(1e-300)
    return float(r.nan_to_num(nan=float("inf")).max())
