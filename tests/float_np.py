"""The float input formats of include/ugsm.h (UGSM_INPUT_RGB32F, UGSM_INPUT_MONO32F) in NumPy and oracle stages, for the tests.

The contract of a float image is the algorithm's own: level 0 of the pyramid IS the given floats (the reference's (float)byte is left
out, nothing else changes).  So the yardstick of a float call is the CPU oracle's stages composed the way tests/seeded_np.py composes the
cold call, started from the float planes instead of from rgb_to_planes of bytes.

    encode(rgb, fmt)                 an (H, W, 3) array of samples -> the image in `fmt`: (H, W, 3) float32, or (H, W) float32 (channel 0)
    planes(img, fmt)                 the image's level 0: (3, H, W) float32 (mono32f: the one channel three times)
    cold_float(orc, L, R, levels)    the field a full-mode call on the planes L, R must write, bit for bit
    colour_byte(v)                   a float sample as the byte of the clouds' colour word
    colour_word(img, fmt)            R << 16 | G << 8 | B of every pixel, (H, W) uint32
"""
import numpy as np

import seeded_np as sn

RGB32F, MONO32F = 8, 9
FORMATS = (RGB32F, MONO32F)
NAMES = {RGB32F: "rgb32f", MONO32F: "mono32f"}
ENCODINGS = {RGB32F: "32FC3", MONO32F: "32FC1"}
BPP = {RGB32F: 12, MONO32F: 4}
EIGHT_BIT = {RGB32F: 0, MONO32F: 4}  # the 8-bit format an integer-valued float image must agree with: rgb8, mono8


def encode(rgb, fmt):
    rgb = np.asarray(rgb)
    assert rgb.ndim == 3 and rgb.shape[2] == 3
    if fmt == RGB32F:
        return np.ascontiguousarray(rgb, np.float32)
    if fmt == MONO32F:
        return np.ascontiguousarray(rgb[..., 0], np.float32)
    raise ValueError(f"not a float format: {fmt}")


def planes(img, fmt):
    img = np.asarray(img, np.float32)
    if fmt == RGB32F:
        return np.ascontiguousarray(img.transpose(2, 0, 1))
    if fmt == MONO32F:
        return np.ascontiguousarray(np.repeat(img[None], 3, axis=0))
    raise ValueError(f"not a float format: {fmt}")


def cold_float(orc, L, R, levels):
    """seeded_np.cold_by_stages from float planes: orc.pyramid of L and R (3, H, W), the zero seed at the top level with its first-iteration
    exception, matchlevel and subsampleDisp down to level 0."""
    pl, pr = orc.pyramid(np.ascontiguousarray(L, np.float32), levels), orc.pyramid(np.ascontiguousarray(R, np.float32), levels)
    return sn.descend(orc, pl, pr, np.zeros_like(pl[levels - 1]), levels - 1, True)


def colour_byte(v):
    """NaN or v <= 0 -> 0, v >= 255 -> 255, else (uint8_t)(v + 0.5f) in binary32."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        mid = np.where((v > 0) & (v < 255), v, np.float32(0))
        b = np.floor(mid + np.float32(0.5)).astype(np.uint32)  # (v + 0.5f >= 0: truncation is floor)
        return np.where(v >= 255, np.uint32(255), np.where(v > 0, b, np.uint32(0))).astype(np.uint32)


def colour_word(img, fmt):
    c = colour_byte(planes(img, fmt))
    return (c[0] << 16) | (c[1] << 8) | c[2]


def rows(img, pad_bytes=0):
    """The image's bytes as rows of a wider buffer: (H, row bytes + pad_bytes) uint8, the padding filled with 0xA5 (a NaN-free pattern is not
    needed: padding is never read)."""
    img = np.ascontiguousarray(img)
    H, row = img.shape[0], img[0].nbytes
    buf = np.full((H, row + pad_bytes), 0xA5, np.uint8)
    buf[:, :row] = img.view(np.uint8).reshape(H, row)
    return buf
