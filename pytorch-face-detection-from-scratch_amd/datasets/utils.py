"""`ReduceBoundingBoxes` and `nms` with the reference's names (datasets/utils.py:95-170):
threshold -> affine decode -> xyxy -> round -> greedy NMS -> xywh, in one HIP launch per batch.
"""
import torch
import torch.nn as nn

from .. import hotpath as hp
from ..hotpath import nms  # noqa: F401  (keyword-compatible stand-in for torchvision.ops.nms)


class ReduceSSDBoundingBoxes(nn.Module):
    """datasets/utils.py:8-92: SSD decode (optionally with priors) -> threshold -> round -> NMS -> xywh."""

    def __init__(self, probability_threshold: float = 0.9, iou_threshold: float = 0.5, input_shape=(3, 320, 240),
                 patch_sizes=(60, 30, 15, 7), priors=None, with_priors=False):
        super().__init__()
        self.priors = priors                                 # (P,4) table or None = calculate_priors() inside the kernel (:31-34)
        self.probability_threshold = probability_threshold
        self.iou_threshold = iou_threshold
        self.input_shape = input_shape
        _, self.width, self.height = input_shape
        self.patch_sizes = tuple(patch_sizes)
        self.with_priors = with_priors

    def forward_batch(self, x: torch.Tensor):
        """(B,P,5) -> (rows (B,P,5) [score,x,y,w,h], counts (B,)), on the GPU, no host sync."""
        return hp.ssd_reduce_bounding_boxes(x, self.probability_threshold, self.iou_threshold, self.width, self.height,
                                            self.patch_sizes, self.with_priors, self.priors)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        rows, counts = self.forward_batch(x.unsqueeze(0))
        k = int(counts[0])
        if k == 0:
            return torch.empty(0).reshape(0, 5)
        return rows[0, :k]


class ReduceBoundingBoxes(nn.Module):
    def __init__(self, probability_threshold: float = 0.9, iou_threshold: float = 0.5,
                 input_shape=(3, 320, 240), num_of_patches=40):
        super().__init__()
        self.probability_threshold = probability_threshold
        self.iou_threshold = iou_threshold
        self.input_shape = input_shape
        _, self.width, self.height = input_shape              # names as in the reference (:107)
        self.x_patch_size = self.width / num_of_patches
        self.y_patch_size = self.height / num_of_patches
        self.num_of_patches = num_of_patches

    def forward_batch(self, x: torch.Tensor):
        """(B,5,S,S) -> (rows (B,S*S,5) [score,x,y,w,h], counts (B,) int32), all on the GPU,
        no host synchronisation."""
        return hp.reduce_bounding_boxes(x, self.probability_threshold, self.iou_threshold, self.width, self.height)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(5,S,S) -> (K',5).  No boxes -> empty (0,5) tensor on the CPU, as the reference
        returns (:170)."""
        rows, counts = self.forward_batch(x.unsqueeze(0))
        k = int(counts[0])
        if k == 0:
            return torch.empty(0).reshape(0, 5)
        return rows[0, :k]


def convert_bbx_to_xyxy(bbx):
    return bbx[0], bbx[1], bbx[0] + bbx[2], bbx[1] + bbx[3]


def outline_width(w, h) -> int:
    """The reference's thickness rule (datasets/utils.py:198-201)."""
    return 1 if (w <= 15 or h <= 15) else 3


@torch.no_grad()
def draw_bbx(img, bbx, input_shape=(320, 240), save_name="image", show=False, save_dir="imgs"):
    """datasets/utils.py:177-210: blue outlines of `bbx` on `img`, saved to `{save_dir}/{save_name}.png` (the reference
    fixes the directory to imgs/; here it is created when missing).  img: a CHW tensor (float in [0,1] -> mul(255).byte(),
    as ToPILImage does, or uint8) or a PIL image.  bbx: a list or tensor of [x,y,w,h] or [score,x,y,w,h] rows, or a raw
    (5,S,S) map, which goes through ReduceBoundingBoxes(0.5, 0.5, (3, *input_shape), S) first (GPU only, as every reducer
    here).  A CUDA image is rendered on the device (`render.render_detections` on a one-image bank; boxes narrower or lower
    than one pixel are skipped), a CPU image with PIL's ImageDraw as the reference does.  show=True is
    refused: there is no display to show it on.  -> the ImageDraw of the saved image."""
    import os
    from PIL import Image, ImageDraw
    if show:
        raise ValueError("draw_bbx: show=True needs a display; the image is saved instead (show=False)")
    bbxs = bbx
    if isinstance(bbxs, torch.Tensor) and bbxs.dim() == 3:
        shape = tuple(int(s) for s in input_shape)[-2:]
        bbxs = ReduceBoundingBoxes(0.5, 0.5, (3, *shape), bbxs.shape[1])(bbxs)
    boxes = [[float(v) for v in b] for b in bbxs]
    boxes = [b[1:] if len(b) == 5 else b for b in boxes]
    if any(len(b) != 4 for b in boxes):
        raise ValueError("draw_bbx: boxes must be [x,y,w,h] or [score,x,y,w,h] rows")
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, f"{save_name}.png")
    if isinstance(img, torch.Tensor):
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError(f"draw_bbx: expected a (3,H,W) image tensor, got {tuple(img.shape)}")
        u8 = img if img.dtype == torch.uint8 else img.mul(255).byte()
        hwc = u8.permute(1, 2, 0).contiguous()
        if hwc.is_cuda:
            import numpy as np
            from ..render import render_detections
            from .augment import IMAGE_DTYPE, DeviceImageBank
            bank = DeviceImageBank(hwc.reshape(-1), np.array([(0, hwc.shape[0], hwc.shape[1])], dtype=IMAGE_DTYPE))
            rows = torch.tensor([[0.0] + b for b in boxes], dtype=torch.float32).reshape(1, len(boxes), 5).to(hwc.device)
            counts = torch.tensor([len(boxes)], dtype=torch.int32, device=hwc.device)
            pil = Image.fromarray(render_detections(bank, rows, counts).to_arrays()[0])
            pil.save(path)
            return ImageDraw.Draw(pil)
        img = Image.fromarray(hwc.numpy())
    draw = ImageDraw.Draw(img)
    for b in boxes:
        draw.rectangle(convert_bbx_to_xyxy(b), outline="blue", width=outline_width(b[2], b[3]))
    img.save(path)
    return draw
