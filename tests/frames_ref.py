"""numpy restatement of gsr_frame_sobel (include/gsr.h, FRAME_SOBEL) in the kernel's own order of operations, float32
throughout: every product and sum below is one rounded numpy operation, so the result is the kernel's bits."""
import numpy as np


def sobel_ordered(image):
    """image float32 [C,H,W] -> float32 [1,H,W]."""
    image = np.asarray(image, np.float32)
    C, H, W = image.shape
    f = np.float32
    acc = np.zeros((H, W), np.float32)
    for c in range(C):
        p = np.zeros((H + 2, W + 2), np.float32)
        p[1:-1, 1:-1] = image[c]
        a0, a1, a2 = p[:-2, :-2], p[:-2, 1:-1], p[:-2, 2:]     # row y - 1 at columns x - 1, x, x + 1
        m0, m2 = p[1:-1, :-2], p[1:-1, 2:]
        b0, b1, b2 = p[2:, :-2], p[2:, 1:-1], p[2:, 2:]
        gx = ((((f(-0.25) * a0 + f(0.25) * a2) + f(-0.5) * m0) + f(0.5) * m2) + f(-0.25) * b0) + f(0.25) * b2
        gy = ((((f(-0.25) * a0 + f(-0.5) * a1) + f(-0.25) * a2) + f(0.25) * b0) + f(0.5) * b1) + f(0.25) * b2
        mag = np.sqrt(gx * gx + gy * gy)
        acc = acc + mag * mag
    out = np.sqrt(acc)
    assert out.dtype == np.float32
    return out[None]
