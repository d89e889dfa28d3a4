"""The waterfall's colours restated in Python integers, from the reference's text.

SpectrumWidget's constructor, application/spectrumwidget.cpp:97-113 (C int arithmetic: every operand is non-negative, so `/` is floor
division), builds m_spectrumColors[i] for i = 0..255 with QColor::setRgb(r, g, b) (alpha 255); drawWaterfall, :1111-1113, paints pixel
value v with m_spectrumColors[255 - v].  A QRgb is 0xAARRGGBB.  The reference allocates 255 entries and touches entry 255 out of
bounds; the table here has all 256, entry 255 being what the loop computes for it (the library's documented deviation).
"""
import numpy as np


def palette_rgb(i):
    """(r, g, b) of m_spectrumColors[i], the constructor's six ranges as written"""
    rgb = None
    if i < 43:
        rgb = (0, 0, 255 * i // 43)
    if 43 <= i < 87:
        rgb = (0, 255 * (i - 43) // 43, 255)
    if 87 <= i < 120:
        rgb = (0, 255, 255 - (255 * (i - 87) // 32))
    if 120 <= i < 154:
        rgb = (255 * (i - 120) // 33, 255, 0)
    if 154 <= i < 217:
        rgb = (255, 255 - (255 * (i - 154) // 62), 0)
    if i >= 217:
        rgb = (255, 0, 128 * (i - 217) // 38)
    return rgb


def palette():
    """uint32 [256]: entry i as 0xFFRRGGBB"""
    out = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        r, g, b = palette_rgb(i)
        out[i] = 0xFF000000 | (r << 16) | (g << 8) | b
    return out


def waterfall(pixels):
    """drawWaterfall's colour of every pixel value (0..255): uint32, same shape"""
    px = np.asarray(pixels)
    assert px.size == 0 or (px.min() >= 0 and px.max() <= 255)
    return palette()[255 - px.astype(np.int64)]
