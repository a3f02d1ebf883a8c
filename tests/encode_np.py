"""The input formats of include/ugsm.h (UGSM_INPUT_*) in NumPy, both ways, for the tests.

A call on an image in format F gives, byte for byte, the rgb8 call's result on that image converted the way cv_bridge converts it to rgb8:
  rgb8  (b0, b1, b2)        bgr8  (b2, b1, b0)
  rgba8 (b0, b1, b2)        bgra8 (b2, b1, b0)          (alpha ignored)
  mono8 (v, v, v)
encode() makes an F image from an rgb8 one (inputs); to_rgb8() is the conversion above (expectations).  A mono8 image made from an rgb8
one keeps channel 0; its conversion is that channel three times.
"""
import numpy as np

RGB8, BGR8, RGBA8, BGRA8, MONO8 = 0, 1, 2, 3, 4
FORMATS = (RGB8, BGR8, RGBA8, BGRA8, MONO8)
NAMES = {RGB8: "rgb8", BGR8: "bgr8", RGBA8: "rgba8", BGRA8: "bgra8", MONO8: "mono8"}
BPP = {RGB8: 3, BGR8: 3, RGBA8: 4, BGRA8: 4, MONO8: 1}


def encode(rgb, fmt, alpha=None):
    """(H, W, 3) uint8 rgb8 -> the image in `fmt`: (H, W) for mono8, (H, W, 3) or (H, W, 4) otherwise.  alpha: (H, W) uint8 or None
    (then a pattern that is not constant, so that a kernel reading it would be caught)."""
    rgb = np.asarray(rgb, np.uint8)
    if fmt == RGB8:
        return rgb.copy()
    if fmt == BGR8:
        return np.ascontiguousarray(rgb[..., ::-1])
    if fmt == MONO8:
        return np.ascontiguousarray(rgb[..., 0])
    if alpha is None:
        H, W = rgb.shape[:2]
        alpha = ((np.arange(H)[:, None] * 37 + np.arange(W)[None, :] * 11 + 5) % 256).astype(np.uint8)
    colour = rgb if fmt == RGBA8 else rgb[..., ::-1]
    return np.ascontiguousarray(np.concatenate([colour, alpha[..., None]], axis=2))


def to_rgb8(img, fmt):
    """An image in `fmt` -> (H, W, 3) uint8 rgb8, as cv_bridge converts it."""
    img = np.asarray(img, np.uint8)
    if fmt == RGB8:
        return np.ascontiguousarray(img)
    if fmt == BGR8:
        return np.ascontiguousarray(img[..., ::-1])
    if fmt == RGBA8:
        return np.ascontiguousarray(img[..., :3])
    if fmt == BGRA8:
        return np.ascontiguousarray(img[..., 2::-1])
    if fmt == MONO8:
        return np.ascontiguousarray(np.repeat(img[..., None], 3, axis=2))
    raise ValueError(f"unknown format {fmt}")


def padded(img, pad_bytes):
    """The image's bytes as rows of a wider buffer: (H, row bytes + pad_bytes) uint8, the padding filled with 0xA5."""
    H = img.shape[0]
    row = img[0].nbytes
    buf = np.full((H, row + pad_bytes), 0xA5, np.uint8)
    buf[:, :row] = np.ascontiguousarray(img).reshape(H, row)
    return buf
