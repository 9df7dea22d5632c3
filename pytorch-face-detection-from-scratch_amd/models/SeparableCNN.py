"""`SeparableCNN` with the reference's constructor, parameter names and forward signature
(models/SeparableCNN.py:10-112).  The nn.Conv2d modules only hold the parameters; the arithmetic runs in the HIP
separable-stack engine (sepstack.py: one fused kernel per residual block).

The reference fixes num_of_patches=16 whatever the head produces: with the default arguments a 480x480 input gives a
10x10 map, which `forward` returns as it is while `ReduceBoundingBoxes` keeps scaling by W/16.  That is reproduced.  The
coherent configurations are those whose head gives 16x16 (480x480 with output_padding=3; 512x512 with
output_kernel_size=1), or the pattern of the reference's pruner.py:32-38:

    model.num_of_patches = 10
    model.reduce_bounding_boxes = ReduceBoundingBoxes(0.5, 0.5, model.input_shape, model.num_of_patches)

(the pooling rule `H > 16` belongs to the blocks and stays as constructed)."""
import torch
import torch.nn as nn

from .. import hotpath as hp
from ..convstack import StackGeometry
from ..sepstack import SepStack, param_names
from .BaseModel import BaseModel


class ResidualBlock(nn.Module):
    """Parameter holder for pointwise_conv1 / depthwise_conv / pointwise_conv2 (no biases); forward lives in the engine."""

    def __init__(self, filters, num_of_patches, dropout=0.25, bias=False):
        super().__init__()
        self.num_of_patches = num_of_patches
        self.pointwise_conv1 = nn.Conv2d(filters, filters, kernel_size=(1, 1), padding=0, bias=bias)
        self.depthwise_conv = nn.Conv2d(filters, filters, kernel_size=(3, 3), padding=1, groups=filters, bias=bias)
        self.pointwise_conv2 = nn.Conv2d(filters, filters, kernel_size=(1, 1), padding=0, bias=bias)
        self.dropout = dropout
        if bias:
            raise hp.N.FdetError("the separable block is built without biases (models/SeparableCNN.py:11), as its zero padding needs")


class SeparableCNN(BaseModel):
    def __init__(self, filters, input_shape, num_of_residual_blocks=10, probability_threshold=0.5, iou_threshold=0.5,
                 pretrained=False, input_kernel_size=10, input_stride=8, output_kernel_size=6, output_padding=0):
        super().__init__(filters, input_shape, num_of_patches=16, probability_threshold=probability_threshold,
                         iou_threshold=iou_threshold)
        self.pretrained = pretrained
        self.conv1 = nn.Conv2d(input_shape[0], filters, kernel_size=(input_kernel_size, input_kernel_size),
                               stride=(input_stride, input_stride), padding=input_kernel_size - input_stride)
        self.residual_blocks = nn.Sequential(
            *[ResidualBlock(filters=filters, num_of_patches=self.num_of_patches) for _ in range(num_of_residual_blocks)])
        self.out = nn.Conv2d(filters, 5, stride=(1, 1), kernel_size=(output_kernel_size, output_kernel_size),
                             padding=output_padding)
        self._stem = (input_kernel_size, input_stride, input_kernel_size - input_stride)
        self._head = (output_kernel_size, output_padding)
        self._pool_above = self.num_of_patches             # the blocks' `H > num_of_patches` rule is fixed at construction
        self._geometry().levels()                          # shapes the engine cannot run fail here, not at the first batch

    def _geometry(self):
        return StackGeometry("separablecnn", self.filters, self.input_shape[0], self.input_shape[1], self.input_shape[2],
                             self._pool_above, len(self.residual_blocks), *self._stem, *self._head, pool_mult=1,
                             strict_grid=False)

    @property
    def engine(self) -> SepStack:
        if self._engine is None:
            self._engine = SepStack(self._geometry())
        return self._engine

    def named_stack_params(self):
        names = param_names(len(self.residual_blocks))
        sd = dict(self.named_parameters())
        return names, [sd[n] for n in names]

    @staticmethod
    def coherent_head(size: int):
        """{output_kernel_size, output_padding} that make a square `size` input reach the 16x16 grid num_of_patches=16
        decodes: k=6, p=3 on a 15x15 last map (480), k=1, p=0 on a 16x16 one (512).  FdetError for any other size."""
        h = (size + 2 * 2 - 10) // 8 + 1                   # the default stem: Conv2d(3, F, 10, stride 8, padding 2)
        while h > 16 and h % 2 == 0:
            h //= 2
        if size % 16 == 0 and h == 15:
            return {"output_kernel_size": 6, "output_padding": 3}
        if size % 16 == 0 and h == 16:
            return {"output_kernel_size": 1, "output_padding": 0}
        raise hp.N.FdetError(f"SeparableCNN at {size}x{size} ends on a {h}x{h} map: no head of the model gives the 16x16 grid its "
                             "decoder assumes (480 and 512 do)")

    def quantize(self, frames_iter, **kw):
        """Int8 post-training quantisation for inference: calibrate the activation scales on `frames_iter` (quantize.calibrate;
        keywords method / percentile) and return the Int8SeparableCNN of this model (64 or 128 filters)."""
        from ..quantize import quantize_model
        return quantize_model(self, frames_iter, **kw)

    def forward(self, x: torch.Tensor, predict: torch.Tensor = torch.tensor(0)):
        if predict == 1:
            x = self.forward_frames(x)
        else:
            x = self._stack_forward(x)
        if predict == 1:
            x = self.single_non_max_suppression(x[0])      # image 0 only, as the reference (:110-111)
        return x
