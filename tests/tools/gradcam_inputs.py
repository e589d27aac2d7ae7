"""Case table of the Grad-CAM fixture (tests/golden/gradcam.npz), shared by the generator
(make_golden_gradcam.py) and the tests.  Inputs are never stored: weights come from
`oracle.unet_ref.fill_state_dict(WEIGHT_SEED)`, images from `synthetic_batch(seed, n, h, w)`, and
the fixture keeps a SHA-256 of both so a test can prove it rebuilt what the reference saw."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WEIGHT_SEED = 31
# name -> (seed, n, h, w) of synthetic_batch
BATCHES = {"sq": (2, 3, 64, 64), "wide": (2, 2, 64, 128)}

# (case name, batch, target layer as (kind, index), class)
CASES = [(f"dec0_c{c}", "sq", ("decoder", 0), c) for c in range(3)] + \
        [(f"enc5_c{c}", "sq", ("encoder", 5), c) for c in range(3)] + \
        [("declast_c1", "sq", ("decoder", -1), 1),
         ("enc0_c1", "sq", ("encoder", 0), 1),
         ("enc3_c1", "sq", ("encoder", 3), 1),
         ("wide_dec2_c2", "wide", ("decoder", 2), 2)]     # 64 x 128: an H / W transposition shows

# the case that holds all-zero and non-zero maps in one batch (per-image normalisation, zero guard)
ZERO_CASE = "enc5_c1"


def layer_key(layer):
    """'decoder_stages[-1]' ... : the key the per-layer error bound is taken over."""
    return f"{layer[0]}_stages[{layer[1]}]"


def target_module(model, layer):
    stages = model.encoder_stages if layer[0] == "encoder" else model.decoder_stages
    return stages[layer[1]]


def state_dict():
    from oracle import unet_ref as O
    return O.fill_state_dict(WEIGHT_SEED)


def images(batch):
    from oracle import unet_ref as O
    seed, n, h, w = BATCHES[batch]
    return O.synthetic_batch(seed, n, h, w)[0]


def digest(sd, imgs):
    """SHA-256 (uint8 [32]) over the weights in key order and every batch in BATCHES order."""
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k].numpy()).tobytes())
    for name in BATCHES:
        h.update(np.ascontiguousarray(imgs[name].numpy()).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def layer_bounds(g):
    """{layer key: bound} from the fixture: max(1e-4, 4 x the largest ref32_err over the layer's
    cases) - the project's logits tolerance, or four times the distance the reference's own fp32
    run keeps from its fp64 run, whichever is larger."""
    worst = {}
    for name, _, layer, _ in CASES:
        k = layer_key(layer)
        worst[k] = max(worst.get(k, 0.0), float(g[f"ref32_err_{name}"]))
    return {k: max(1e-4, 4.0 * v) for k, v in worst.items()}
