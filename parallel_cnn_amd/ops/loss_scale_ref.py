"""Pure-Python reference of the DeepCNN loss scaler (k_ls_advance,
csrc/hip/conv_kernels.hip): the state words, Adam's bias corrections as the
device forms them, and the advance rule.  The engine initialises the device
state from here; the tests hold the kernel to it bit for bit."""
from __future__ import annotations

import math
import struct

LS_MIN_SCALE = 1.0
LS_MAX_SCALE = 2.0 ** 24


def _f32(v: float) -> float:
    """v rounded to float32 (what a state word holds)."""
    return struct.unpack("f", struct.pack("f", v))[0]


def _ipow(b: float, t: int) -> float:
    """b**t by repeated squaring, double products in the order k_ls_advance
    forms them (a library pow promises no particular last bit)."""
    r = 1.0
    while t > 0:
        if t & 1:
            r = r * b
        b = b * b
        t >>= 1
    return r


def adam_corrections(beta1: float, beta2: float, t: int):
    """(c1, c2) of the 1-based update t, formed in double and rounded to
    float32: c1 = 1/(1-beta1^t), c2 = 1/sqrt(1-beta2^t)."""
    return (_f32(1.0 / (1.0 - _ipow(beta1, t))),
            _f32(1.0 / math.sqrt(1.0 - _ipow(beta2, t))))


def scaler_state(scale: float, beta1: float = 0.0, beta2: float = 0.0,
                 good_steps: int = 0, skipped: int = 0, t: int = 1) -> dict:
    """A loss scaler's state as the device buffer holds it.  t is the 1-based
    count of the NEXT update, the one c1 and c2 belong to."""
    c1, c2 = adam_corrections(beta1, beta2, t)
    return {"scale": float(scale), "inv_scale": 1.0 / float(scale),
            "found_inf": 0, "good_steps": good_steps, "skipped": skipped,
            "t": t, "c1": c1, "c2": c2}


def advance_reference(state: dict, found_inf: bool, growth_interval: int,
                      dynamic: bool = True, beta1: float = 0.0,
                      beta2: float = 0.0) -> dict:
    """Pure-Python reference of k_ls_advance: the state after one step whose
    overflow check said found_inf.  Overflow: the step was skipped -- scale
    halves (floor 1), good_steps restarts, skipped counts it, and t, c1, c2
    stay.  Otherwise t moves on, c1 and c2 are recomputed in double for the
    next update, and after growth_interval applied updates in a row the scale
    doubles (ceiling 2^24).  A fixed scale (dynamic=False) never moves and
    keeps good_steps at rest; skips are still counted."""
    s = dict(state)
    if found_inf:
        s["skipped"] += 1
        if dynamic:
            s["scale"] = max(0.5 * s["scale"], LS_MIN_SCALE)
            s["good_steps"] = 0
    else:
        s["t"] += 1
        s["c1"], s["c2"] = adam_corrections(beta1, beta2, s["t"])
        if dynamic:
            s["good_steps"] += 1
            if s["good_steps"] >= growth_interval:
                s["scale"] = min(2.0 * s["scale"], LS_MAX_SCALE)
                s["good_steps"] = 0
    s["inv_scale"] = 1.0 / s["scale"]
    s["found_inf"] = 0
    return s
