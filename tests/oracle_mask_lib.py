"""numpy restatements of what --ignore-mask-label does before the estimate: the label list (Util::strSplit + atoi), cv::resize
INTER_NEAREST of the label image (OpenCV's resizeNN) and the keep-mask they give.  The masked estimate itself is the oracle's
(oracle_lib.estimate(keep=...)).  Test infrastructure only."""
import re

import numpy as np


def parse_labels(arg):
    """--ignore-mask-label: Util::strSplit(s, ",") keeping empty tokens (libs/Common/Util.h:530-545), each token through atoi
    (DepthMap.cpp:319-348).  An empty string means no mask at all (None)."""
    if not arg:
        return None
    return [atoi(t) for t in arg.split(",")]


def atoi(t):
    """C atoi: leading blanks, an optional sign, the digits that follow; 0 when there are none (the value wraps to int32 as glibc's
    strtol-based atoi does for what fits in a long)"""
    m = re.match(r"\s*([+-]?\d+)", t)
    if not m:
        return 0
    v = int(m.group(1))
    v = max(min(v, (1 << 63) - 1), -(1 << 63))       # strtol saturates to LONG_MIN / LONG_MAX
    return ((v + (1 << 31)) % (1 << 32)) - (1 << 31)  # (int) of the long


def resize_nn(labels, w, h):
    """cv::resize(labels, Size(w, h), 0, 0, INTER_NEAREST): resizeNN with ifx = 1 / (w / sw), sx = min(floor(x * ifx), sw - 1)"""
    lab = np.asarray(labels)
    sh, sw = lab.shape
    if (sw, sh) == (w, h):
        return lab.copy()
    ifx = 1.0 / (w / sw); ify = 1.0 / (h / sh)
    sx = np.minimum(np.floor(np.arange(w, dtype=np.float64) * ifx).astype(np.int64), sw - 1)
    sy = np.minimum(np.floor(np.arange(h, dtype=np.float64) * ify).astype(np.int64), sh - 1)
    return lab[sy[:, None], sx[None, :]]


def keep_mask(labels, ignore, w, h):
    """DepthEstimator::ImportIgnoreMask: 1 where the resampled label equals none of the ignored labels"""
    r = resize_nn(np.asarray(labels, np.uint16), w, h).astype(np.int64)
    keep = np.ones((h, w), np.uint8)
    for v in ignore or []:
        keep[r == int(v)] = 0
    return keep


def median3_window_valid(keep, depth_init):
    """per pixel: how many of the 9 values of its 3x3 median window (edges replicated, as medianBlur does) come from pixels that are
    not ignored and hold a positive initial depth"""
    h, w = keep.shape
    ok = ((keep != 0) & (np.asarray(depth_init) > 0)).astype(np.int32)
    pad = np.pad(ok, 1, mode="edge")
    return sum(pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
