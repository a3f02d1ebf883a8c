"""Images that leave K-cost's guarded-division range, in NumPy, for the tests.

The fused kernels divide with div_inrange (csrc/ugsm_exact.hpp) while every pyramid value of a pair passes range_ok:
v == 0 or 2^-12 <= v <= 2^9.  A synth.make_pair image is quantised to [1, 255] and never leaves that range at any level; the ordinary
camera images below do: a dim pixel on black is blurred and decimated to 8.16e-3 at levels 1 and 2 (still in range) and to
6.7e-5 < 2^-12 at level 3, then on down to 1e-8.  Every recipe takes an (H, W, 3) uint8 rgb8 image and returns a changed copy.

out_of_range_levels counts, per pyramid level of the CPU oracle, the values outside the range with the literal predicate: the premise
every test asserts before it believes a word read back from the device.
"""
import numpy as np

RANGE_LO = 2.0 ** -12
RANGE_HI = 2.0 ** 9


def dark_noise(img, seed, frac=1.0 / 3.0, density=0.002):
    """The left `frac` of the columns black except `density` of its pixels, which hold 1..3 in every channel: sensor noise in the dark."""
    out = np.array(img, np.uint8, copy=True)
    H, W = out.shape[:2]
    wd = max(1, int(W * frac))
    rng = np.random.Generator(np.random.PCG64(seed))
    lit = rng.random((H, wd)) < density
    val = rng.integers(1, 4, (H, wd, 3), dtype=np.uint8)
    out[:, :wd] = np.where(lit[..., None], val, np.uint8(0))
    return out


def black_frame(img, rows=12, right=16):
    """`rows` black rows at the top and at the bottom, `right` black columns at the right: a rectified image's border."""
    out = np.array(img, np.uint8, copy=True)
    out[:rows] = 0
    out[out.shape[0] - rows:] = 0
    out[:, out.shape[1] - right:] = 0
    return out


def saturated_block(img, y0, x0, h=60, w=70):
    """An h x w block of 255 with its corner at (y0, x0): a blown-out highlight."""
    out = np.array(img, np.uint8, copy=True)
    out[y0:y0 + h, x0:x0 + w] = 255
    return out


def one_dim_pixel(img, block=64, value=1, centre=None):
    """A block x block black square around `centre` = (y, x) (default: the image's centre) with one (value, value, value) pixel at the centre."""
    out = np.array(img, np.uint8, copy=True)
    H, W = out.shape[:2]
    cy, cx = centre if centre is not None else (H // 2, W // 2)
    y0, x0 = max(0, cy - block // 2), max(0, cx - block // 2)
    out[y0:y0 + block, x0:x0 + block] = 0
    out[cy, cx] = value
    return out


def dark_image(img, seed):
    """dark_noise + black_frame + saturated_block on one image: the dark, noisy, framed and partly blown-out camera image."""
    H, W = img.shape[:2]
    return saturated_block(black_frame(dark_noise(img, seed)), H // 2, (2 * W) // 3 - 35,
                           h=min(60, H // 4), w=min(70, W // 4))


def dark_pair(L, R, seed):
    """dark_image on both images of a pair, with different noise."""
    return dark_image(L, seed), dark_image(R, seed + 1)


def degenerate_pairs(L, R):
    """name -> (left, right): all 0, all 255, constant 7, L black / R textured, L textured / R black."""
    z, s, c = np.zeros_like(L), np.full_like(L, 255), np.full_like(L, 7)
    return {"all 0": (z, z.copy()), "all 255": (s, s.copy()), "constant 7": (c, c.copy()),
            "L black, R textured": (z.copy(), np.array(R, copy=True)), "L textured, R black": (np.array(L, copy=True), z.copy())}


def in_range(v):
    """range_ok of csrc/ugsm_exact.hpp, literally, elementwise (a NaN is out of range)."""
    v = np.asarray(v, np.float32)
    return (v == 0) | ((v >= np.float32(RANGE_LO)) & (v <= np.float32(RANGE_HI)))


def out_of_range_levels(orc, img, levels):
    """Per pyramid level of the oracle's pyramid of `img`: how many values fail range_ok."""
    pyr = orc.pyramid(orc.rgb_to_planes(np.ascontiguousarray(img)), levels)
    return [int((~in_range(p)).sum()) for p in pyr]


def trips(counts):
    """The premise of a tripping image: out-of-range values at some level >= 3 (levels 0-2 of an 8-bit image cannot hold one)."""
    return sum(counts[3:]) > 0 and sum(counts[:3]) == 0


def pair_word(orc, L, R, levels):
    """The range word the device must report for the pair (1 or 0) and the per-level counts behind it, (word, countsL, countsR)."""
    cl, cr = out_of_range_levels(orc, L, levels), out_of_range_levels(orc, R, levels)
    return int(sum(cl) + sum(cr) > 0), cl, cr


def kcost_operands(orc, L3, R3):
    """The operand pairs (N^2, A*B) of K-cost's 15 divisions per pixel of one level at zero disparity (R' = R), restated from the oracle's
    iterate_level: A = G_clamp * L^2, B = G_clamp * R^2, N = G_zero * (L * R shifted by one of the five moves), den = A * B shifted.
    L3, R3: (3, H, W) float32 level images.  Returns (num, den), float32, 15 * H * W each."""
    g = orc.gauss_taps()
    f32 = np.float32
    num, den = [], []

    def shift(a, sx, sy):      # a(x + sx, y + sy), clamp addressed
        H, W = a.shape
        return a[np.clip(np.arange(H) + sy, 0, H - 1)][:, np.clip(np.arange(W) + sx, 0, W - 1)]

    for k in range(3):
        Lk, Rk = np.ascontiguousarray(L3[k], f32), np.ascontiguousarray(R3[k], f32)
        A, B = orc.conv(Lk * Lk, g, "clamp"), orc.conv(Rk * Rk, g, "clamp")
        for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1), (0, 0)):
            N = orc.conv(np.ascontiguousarray(Lk * shift(Rk, sx, sy)), g, "zero")
            num.append((N * N).astype(f32).ravel())
            den.append((A * shift(B, sx, sy)).astype(f32).ravel())
    return np.concatenate(num), np.concatenate(den)
