"""What the JPEG round-trip tests share: the integer specification of DESIGN section 11g as a numpy oracle, the case table and a
restatement of the reference's path (``to_pil_image`` -> PIL JPEG at 4:2:0 -> ``to_tensor``; torchvision's two functions are
restated because torchvision is not a dependency).

The oracle equals PIL (libjpeg-turbo) bit for bit at every size and quality (DESIGN section 11g has the sweep).  It is int64 by
default; ``oracle(..., itype=np.int32)`` runs the same steps in wrapping int32, which is what the kernel
has (tests/test_jpeg_host.py compares the two on the inputs with the largest intermediates)."""
import io

import numpy as np
import torch

# Annex K of the JPEG standard, natural (row-major) order
LUMA_BASE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    dtype=np.int64).reshape(8, 8)
CHROMA_BASE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99],
    dtype=np.int64).reshape(8, 8)

QUALITIES = (1, 10, 49, 50, 75, 95, 100)       # both scaling branches (q < 50, q >= 50) and both clamps (255 at q = 1, 1 at q = 100)

# name -> (shape, qualities).  Each shape is the smallest for what it catches:
CASES = {
    "one_mb": ((1, 3, 16, 16), QUALITIES),               # one macroblock; every quality
    "halo": ((2, 3, 48, 80), (10, 75)),                  # interior chroma halo across macroblock borders, both axes; two frames
    "odd": ((1, 3, 37, 53), (49, 95)),                   # odd ragged size
    "plus_one": ((1, 3, 17, 33), (1, 50)),               # one pixel into a new macroblock
    "batch": ((3, 3, 64, 64), (50, 100)),                # batch
    "even_30": ((1, 3, 30, 18), (10, 95)),               # even ragged heights: the chroma PLANE is replicated below the image (step 4)
    "even_8": ((1, 3, 8, 24), (49, 75)),
    "pixel": ((1, 3, 1, 1), (1, 100)),                   # degenerate planes: chroma at most 2 wide is upsampled by replication (step 9)
    "two_wide": ((1, 3, 16, 2), (50, 75)),
}


def fix(v):
    return int(v * 65536 + 0.5)


def quant_tables(q):
    """(luminance, chrominance) 8 x 8 tables of quality ``q`` (clamped to 1..100), natural order"""
    q = min(max(int(q), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA_BASE, CHROMA_BASE))


def case_input(name, dtype=torch.float32):
    """Smooth structure plus noise, with saturated patches (exact 0 and 1) and values outside [0, 1]: the same tensor on every call"""
    shape = CASES[name][0]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    n, _, h, w = shape
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    ph = torch.rand(n, 3, 1, 1, generator=g) * 6.28
    x = 0.5 + 0.35 * torch.sin(yy * 0.21 + xx * 0.13 + ph) + 0.25 * (torch.rand(shape, generator=g) - 0.5)
    x = torch.where(torch.rand(shape, generator=g) < 0.03, torch.round(torch.rand(shape, generator=g)), x)
    return x.clamp(0, 1).to(dtype)


def to_u8(x):
    """step 1: ``clamp(x, 0, 1) * 255`` formed in the tensor's own dtype, then truncated (``to_pil_image``'s ``mul(255).byte()``)"""
    return x.detach().clamp(0, 1).mul(255).to(torch.uint8).cpu().numpy()


def _D(x, n):
    return (x + (1 << (n - 1))) >> n


def _odd_part(t4, t5, t6, t7):
    """the odd halves of FDCT and IDCT share this: returns (t4', t5', t6', t7') = the four sums before the descale"""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _fdct_pass(d, first):
    """one 1-D pass along the last axis (length 8)"""
    d = [d[..., i] for i in range(8)]
    t0, t1, t2, t3 = d[0] + d[7], d[1] + d[6], d[2] + d[5], d[3] + d[4]
    t7, t6, t5, t4 = d[0] - d[7], d[1] - d[6], d[2] - d[5], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _D(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _D(t10 - t11, 2)
    z = (t12 + t13) * 4433
    o[2] = _D(z + t13 * 6270, n)
    o[6] = _D(z - t12 * 15137, n)
    o[7], o[5], o[3], o[1] = (_D(v, n) for v in _odd_part(t4, t5, t6, t7))
    return np.stack(o, axis=-1)


def _idct_pass(x, n):
    x = [x[..., i] for i in range(8)]
    z1 = (x[2] + x[6]) * 4433
    t2, t3 = z1 - x[6] * 15137, z1 + x[2] * 6270
    t0, t1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = _odd_part(x[7], x[5], x[3], x[1])
    o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_D(v, n) for v in o], axis=-1)


def codec_plane(p, Q, max_abs=None):
    """(N, Hp, Wp) samples 0..255, Hp and Wp multiples of 8 -> the same after FDCT, quantise, dequantise, IDCT per 8 x 8 block.
    ``max_abs``: a one-element list that collects the largest |coefficient| entering the quantiser."""
    n, hp, wp = p.shape
    b = p.reshape(n, hp // 8, 8, wp // 8, 8).transpose(0, 1, 3, 2, 4) - 128          # (..., row, col)
    c = _fdct_pass(b, True)                                                          # over rows: along the columns of each row
    c = _fdct_pass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)
    if max_abs is not None:
        max_abs[0] = max(max_abs[0], int(np.abs(c).max()))
    q8 = Q.astype(p.dtype) * 8
    c = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8) * Q.astype(p.dtype)
    c = _idct_pass(c.swapaxes(-1, -2), 11).swapaxes(-1, -2)                          # columns first
    c = _idct_pass(c, 18)
    c = np.clip(c + 128, 0, 255)
    return c.transpose(0, 1, 3, 2, 4).reshape(n, hp, wp)


def oracle(u8, quality, itype=np.int64, max_abs=None):
    """The specification, steps 2 to 10, on a (N, 3, H, W) uint8 array; returns the same shape, uint8."""
    n, _, h, w = u8.shape
    hp, wp = -(-h // 16) * 16, -(-w // 16) * 16
    x = np.pad(u8.astype(itype), ((0, 0), (0, 0), (0, hp - h), (0, wp - w)), mode="edge")
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    half, off = 1 << 15, 128 << 16
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + half) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + off + half - 1) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + off + half - 1) >> 16
    bias = np.tile(np.array([1, 2], dtype=itype), wp // 4)

    def down(c):
        return (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + bias) >> 2

    ql, qc = quant_tables(quality)
    y = codec_plane(y, ql, max_abs)[:, :h, :w]
    ch, cw = -(-h // 2), -(-w // 2)
    planes = []
    for c in (cb, cr):
        c = down(c)
        c[:, ch:] = c[:, ch - 1:ch]            # below the image the chroma PLANE is replicated, not the pixels under it
        c = codec_plane(c, qc, max_abs)[:, :ch, :cw]
        if cw <= 2:                            # a chroma plane this narrow is upsampled by replication
            planes.append(np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)[:, :h, :w] - 128)
            continue
        c = np.pad(c, ((0, 0), (1, 1), (1, 1)), mode="edge")
        near = c[:, 1:-1]
        v = np.empty((n, 2 * ch, cw + 2), dtype=itype)
        v[:, 0::2] = 3 * near + c[:, :-2]
        v[:, 1::2] = 3 * near + c[:, 2:]
        mid = v[:, :, 1:-1]
        o = np.empty((n, 2 * ch, 2 * cw), dtype=itype)
        o[:, :, 0::2] = (3 * mid + v[:, :, :-2] + 8) >> 4
        o[:, :, 1::2] = (3 * mid + v[:, :, 2:] + 7) >> 4
        planes.append(o[:, :h, :w] - 128)
    cb, cr = planes
    r = y + ((fix(1.402) * cr + half) >> 16)
    b = y + ((fix(1.772) * cb + half) >> 16)
    g = y + ((-fix(.34414) * cb - fix(.71414) * cr + half) >> 16)
    return np.clip(np.stack([r, g, b], axis=1), 0, 255).astype(np.uint8)


def expected(x, quality):
    """what ``jpeg_compress(x, quality)`` must return, bit for bit: the oracle's bytes / 255 in fp32, cast to the dtype of ``x``"""
    squeeze = x.dim() == 3
    u8 = oracle(to_u8(x[None] if squeeze else x), quality)
    out = (torch.from_numpy(u8).to(torch.float32) / 255).to(x.dtype)
    return out[0] if squeeze else out


# ---- the reference's path, restated ----------------------------------------------------------------------------------------
def pil_has_jpeg():
    try:
        from PIL import features
        return bool(features.check("jpg"))
    except Exception:
        return False


def to_pil_image(t):
    """torchvision.transforms.functional.to_pil_image for a float (3, H, W) tensor"""
    from PIL import Image
    return Image.fromarray(np.ascontiguousarray(t.mul(255).byte().permute(1, 2, 0).cpu().numpy()), mode="RGB")


def to_tensor(img):
    """torchvision.transforms.functional.to_tensor for an 8-bit RGB image"""
    a = np.asarray(img, dtype=np.uint8)
    return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def reference_path(x, quality):
    """RandomJPEGCompression.forward of the reference for a fixed quality, on a (N, 3, H, W) tensor"""
    from PIL import Image
    x = x.detach().clamp(0, 1)
    out = []
    for frame in x:
        with io.BytesIO() as buf:
            to_pil_image(frame).save(buf, format="JPEG", quality=quality)
            buf.seek(0)
            with Image.open(buf) as im:
                im.load()
                out.append(to_tensor(im).type_as(frame))
    return torch.stack(out)
