"""bridgeqa_amd -- MI355X-native implementation of BridgeQA's data-parallel hot path.

Host code is Python on PyTorch-ROCm (device memory, streams, torch.distributed only); the
operators are hand-written HIP kernels for gfx950 behind the C ABI of include/bqhip.h
(bridgeqa_amd/lib/libbqhip.so).  Module and operator names mirror the reference
(matthewdm0816/BridgeQA) so the path drops into its scripts/train.py -- see INTEGRATION.md.
"""
__version__ = "0.1.0"

import os as _os

# ---- the deterministic training mode (README "Environment variables") ------------------------------------------
# Off by default: the kernels of a training step are then what they were without the mode, but for one launch -- the LM head's
# dH, the first gradient of the backward, which every other gradient descends from, is summed in piece order in every mode
# (fusion_ops._LMHeadCE.backward).  On: the fusion
# backward's fp32 sums that several workgroups used to add with float atomics (LayerNorm dgamma / dbeta, grouped bias column sums,
# cut contractions such as the LM head's dH) are stored as per-workgroup partials and folded in a fixed order, so that a step
# started from the same parameters, buffers, batch and seed (manual_seed) gives the same bits every time.
_DETERMINISTIC = [_os.environ.get("BQ_DETERMINISTIC", "0") == "1"]


def set_deterministic(flag):
    """switch the deterministic training mode on or off; returns the previous value.  Captured graphs (graphed.enable,
    pipeline.PhasedTrainStep) are captured again at their next step after a change."""
    prev = _DETERMINISTIC[0]
    _DETERMINISTIC[0] = bool(flag)
    return prev


def is_deterministic():
    """True while the deterministic training mode is on (default: the environment variable BQ_DETERMINISTIC=1 at import)"""
    return _DETERMINISTIC[0]


def manual_seed(seed, device=None):
    """torch.manual_seed(seed) and a reset of every dropout / drop-path source of the HIP path: the device-resident step
    counter of fusion_ops (filled IN PLACE: captured graphs hold its address) and the per-call seed counter.  Two executions
    of a step that each start with the same manual_seed draw the same masks, whatever the mode."""
    import torch
    torch.manual_seed(seed)
    from . import fusion_ops
    fusion_ops.reset_seeds(seed, device)
