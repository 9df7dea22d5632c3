#!/usr/bin/env python3
"""Generate the trained Resnet-medium fixture tests/golden/g22_trained_resnet_medium*.npz by RUNNING THE REFERENCE'S OWN
`Resnet` on the CPU (the pattern of tools/make_goldens.py::g6_trained and make_goldens_r4.py::trained_medium).

Run in the build container only (needs the reference checkout, which never travels to the GPU box):
    python tools/make_goldens_resnet.py

  weights   `saved_models/official/Resnet/medium_model_15x15_480.pth` (F = 64, ten blocks, 480 x 480, S = 15), read as raw bytes
            with make_goldens.read_archive_tensors: nothing is unpickled or executed from the archive
  y, dets   the reference class on the three frames already stored in g6_trained_small.npz (`images`); the frames are NOT
            stored again

The archive is 2.9 MB of fp32 and a committed file stays under 1 MiB, so the tensors are spread over four files (three
residual blocks each; conv1, out, y, dets and ndets in the first).  tests/q8_resnet_cpu_ref.py::load_g22 puts them together.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_goldens as MG  # noqa: E402

PARTS = ("g22_trained_resnet_medium", "g22_trained_resnet_medium_b", "g22_trained_resnet_medium_c", "g22_trained_resnet_medium_d")
BLOCKS_PER_PART = 3
LIMIT = 1 << 20


def trained_resnet_medium(R):
    z = np.load(os.path.join(MG.OUT, "g6_trained_small.npz"))
    images = torch.from_numpy(z["images"])
    path = os.path.join(MG.REF, "saved_models/official/Resnet/medium_model_15x15_480.pth")
    P, F_, nb = MG.read_archive_tensors(path)
    assert F_ == 64 and nb == 10 and P["conv1.weight"].shape == (64, 3, 3, 3) and P["out.weight"].shape == (5, 64, 3, 3)
    model = R["Resnet"](filters=F_, input_shape=(3, 480, 480), num_of_patches=15, num_of_residual_blocks=nb,
                        probability_threshold=0.7, iou_threshold=0.01)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    model.eval()
    outs, dets, nd = [], [], []
    for i in range(images.shape[0]):
        u8 = images[i]
        with torch.no_grad():
            yv = model(torch.stack([u8, u8]).float() / 255.0)
            det = model(torch.stack([u8, u8]), predict=torch.tensor(1))
        outs.append(yv[0])
        d = torch.zeros(100, 5); d[: det.shape[0]] = det
        dets.append(d); nd.append(det.shape[0])
        print("resnet medium image", i, "dets", det.shape[0], det[:3].tolist())
    first = dict(y=torch.stack(outs), dets=torch.stack(dets), ndets=np.array(nd), images_from=np.array("g6_trained_small.npz"))
    for k in ("conv1.weight", "conv1.bias", "out.weight", "out.bias"):
        first["param/" + k] = P[k]
    for p, name in enumerate(PARTS):
        arrays = first if p == 0 else {}
        for k in range(p * BLOCKS_PER_PART, min(nb, (p + 1) * BLOCKS_PER_PART)):
            for leaf in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"):
                arrays[f"param/residual_blocks.{k}.{leaf}"] = P[f"residual_blocks.{k}.{leaf}"]
        MG.save(name, **arrays)
        size = os.path.getsize(os.path.join(MG.OUT, name + ".npz"))
        assert size < LIMIT, (name, size)
        print(name, size, "bytes")


if __name__ == "__main__":
    torch.set_num_threads(16)
    trained_resnet_medium(MG.import_reference())
    print("done")
