"""Per-layer recovery from fp16-split range events.

The fp16-split convolutions clamp nothing: when a coefficient / bound call finds that a GroupNorm-ed operand MAY leave fp16's
range it raises EVC_RANGE_F16_OPERAND (include/evc_hip.h), in the device's sticky word and -- inside the score network -- in
the word of its event SITE.  With recovery on, a generated chunk whose site words name such sites is not given up: those
sites are demoted (``ScoreNet.demote``: their consumers move to the exact bf16 split), the noise sources are put back where
they were before the chunk, and the chunk is generated again.  One pass is not always enough (the NaN of the first overflow
makes every later site report EVC_RANGE_NONFINITE and so hides later overflowing layers), so passes repeat until the chunk is
clean; every pass must demote at least one new site, and a non-finite result left without a site to demote is refused with
``NumericsError`` as without recovery.
"""
import os

import torch

MODES = ("off", "layer")
RANGE_NONFINITE, RANGE_F16_OPERAND = 1, 2      # include/evc_hip.h EVC_RANGE_* (lib.RANGE_*)


class NumericsError(RuntimeError):
    pass


def recovery_mode(value=None):
    """``value`` (a --range-recovery argument), else EVC_RANGE_RECOVERY, else "off"."""
    v = (value if value is not None else os.environ.get("EVC_RANGE_RECOVERY", "off")).lower()
    if v not in MODES:
        raise ValueError(f"range recovery must be one of {MODES}, got {v!r}")
    return v


def supports_recovery(net):
    """Networks with event sites and ``demote`` (the unetmore score networks, SPADE included)."""
    return bool(getattr(net, "sites", None)) and hasattr(net, "demote")


def _device_reader(net):
    from . import lib as L

    def read():
        return L.site_events(net, reset=True), L.range_events(net.site_words.device, reset=True)
    return read


def generate_with_recovery(run, restore, net, where="", log=print, read=None):
    """run() -> the chunk (a tensor that must come out finite); restore() puts every noise source back to its state before
    the first run().  ``read()`` -> ({site: bits}, device-word bits), both cleared by the read (default: the device words
    of ``net``).  Returns (chunk, passes, newly demoted sites).  The device word keeps what it held before the call plus what
    the accepted pass raised."""
    prior = 0
    if read is None:
        from . import lib as L
        prior = L.range_events(net.site_words.device, reset=True)
        read = _device_reader(net)
    new_sites = []
    passes = 0
    try:
        while True:
            out = run()
            passes += 1
            sites, glob = read()
            demoted = set(net.demoted_sites())
            over = sorted(k for k, b in sites.items() if b & RANGE_F16_OPERAND and k not in demoted)
            if over:
                net.demote(over)
                new_sites += over
                restore()
                continue
            nonfinite = any(b & RANGE_NONFINITE for b in sites.values())
            finite = bool(torch.isfinite(out).all())
            if glob or nonfinite or not finite:
                raise NumericsError(
                    f"{where}: range recovery pass {passes}: range-event word {glob:#x}, site words "
                    f"{ {k: hex(b) for k, b in sites.items()} }, chunk finite: {finite}, and no site left to demote -- a tensor "
                    f"held NaN / inf that no fp16-split operand explains (e.g. non-finite conditioning frames)")
            break
    finally:
        if prior:
            from . import lib as L
            L.raise_range_events(prior, net.site_words.device)
    if new_sites:
        names = net.demoted_sites()
        log(f"range recovery: {where}: demoted {', '.join(f'{names[k]} (site {k})' for k in new_sites)} to the bf16x6 "
            f"split; chunk clean after {passes} passes (repack time so far {1e3 * getattr(net, 'demote_seconds', 0.0):.1f} ms)")
    return out, passes, new_sites
