#!/usr/bin/env python3
"""Generates tests/golden/lpips_pins.npz by IMPORTING THE REFERENCE's own LPIPS class (read-only checkout beside this repository) on the CPU -- it
does not travel to the GPU box, so the figures it produces are committed, as make_eval_golden.py's are.

    python tests/golden/make_lpips_pins.py

The reference needs torchvision and two downloads; neither exists here, and neither is needed to pin its ARITHMETIC:
  * `torchvision.models` is a stand-in whose alexnet() / vgg16() carry an nn.Sequential `features` built from the layer tables of
    tests/lpips_cases.py (positions, shapes, strides, paddings, the final pools included), loaded with that file's seeded test weights;
  * `get_state_dict` is replaced by one that hands over that file's seeded linear layers under the names the reference's renaming produces.
Everything else -- z-score, taps, normalisation, the 1x1 layers, the mean, the concatenation along the batch axis and its sum -- is the
reference's code, run in .double().  Per case of lpips_cases.NET_CASES the file holds

    <case>_total   the module's output, ()          <case>_terms   (5,): each linear layer's output, averaged over H and W and summed over the batch
    <case>_seed    the seed the weights and the pair were made from (no weights are stored: a few KB)

tests/test_lpips_cpu.py holds the fp64 restatement of tests/lpips_cases.py to these within 1e-12 relative.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

import lpips_cases as LC  # noqa: E402


def _sequential(net):
    layers = []
    for layer in LC.FEATURES[net]:
        if layer[0] == "conv":
            layers.append(nn.Conv2d(layer[1], layer[2], layer[3], layer[4], layer[5]))
        elif layer[0] == "relu":
            layers.append(nn.ReLU(inplace=True))
        else:
            layers.append(nn.MaxPool2d(layer[1], layer[2]))
    return nn.Sequential(*layers)


def _stand_in_torchvision():
    models = types.ModuleType("torchvision.models")
    holder = lambda net: (lambda *a, **k: types.SimpleNamespace(features=_sequential(net)))
    models.alexnet, models.vgg16, models.squeezenet1_1 = holder("alex"), holder("vgg"), None
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    tv = types.ModuleType("torchvision")
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models


def main():
    _stand_in_torchvision()
    from lpipsPyTorch.modules import lpips as ref_lpips  # noqa: E402  (the reference's module)

    out = {}
    for name, (net, B, H, W, seed) in LC.NET_CASES.items():
        backbone, lin = LC.make_weights(net, seed)
        ref_lpips.get_state_dict = lambda net_type, version: {k.replace("lin", "").replace("model.", ""): torch.from_numpy(v) for k, v in lin.items()}
        m = ref_lpips.LPIPS(net, "0.1")
        m.net.layers.load_state_dict({k[len("features."):]: torch.from_numpy(v) for k, v in backbone.items()})
        m = m.double().eval()
        seen = []
        hooks = [l.register_forward_hook(lambda mod, inp, res: seen.append(res.mean((2, 3)).sum())) for l in m.lin]
        x, y = (torch.from_numpy(a).double() for a in LC.make_inputs(B, H, W, seed))
        with torch.no_grad():
            total = m(x, y)
        for h in hooks:
            h.remove()
        assert tuple(total.shape) == (1, 1, 1, 1) and len(seen) == 5
        out[name + "_total"] = total.reshape(()).numpy()
        out[name + "_terms"] = torch.stack(seen).numpy()
        out[name + "_seed"] = np.int64(seed)
        print(name, float(total), out[name + "_terms"])
    path = os.path.join(HERE, "lpips_pins.npz")
    np.savez_compressed(path, **out)
    print("lpips_pins.npz", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
