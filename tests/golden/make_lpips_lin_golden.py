"""Writes tests/golden/lpips_vgg_lin.npz and lpips_squeeze_lin.npz: the trained linear layers of LPIPS-VGG16 and LPIPS-SqueezeNet
v0.1 as the reference ships them (weights/v0.1/vgg.pth and squeeze.pth; identical copies under models/weights and
benchmark/weights), in the manner of lpips_alex_lin.npz (make_goldens.py::gen_lpips_lin).  The files were saved from a CUDA
device: read with the weights-only loader onto the CPU.  Five vectors of 64, 128, 256, 512, 512 floats (1 472) and seven of
64, 128, 256, 384, 384, 512, 512 (2 240).  The backbones they sit on are torchvision's checkpoints, which the reference does not hold.

    python tests/golden/make_lpips_lin_golden.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LAYERS = {"vgg": 5, "squeeze": 7}


def main(ref):
    for net, n in LAYERS.items():
        sd = torch.load(os.path.join(ref, "weights", "v0.1", f"{net}.pth"), map_location="cpu", weights_only=True)
        arrays = {f"lin{i}": sd[f"lin{i}.model.1.weight"].reshape(-1).numpy().astype(np.float32) for i in range(n)}
        np.savez(os.path.join(HERE, f"lpips_{net}_lin.npz"), **arrays)
        print(net, {k: v.shape for k, v in arrays.items()}, sum(v.size for v in arrays.values()), "floats")


if __name__ == "__main__":
    main(sys.argv[1])
