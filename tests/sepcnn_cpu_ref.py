"""CPU restatement of models/SeparableCNN.py (plain torch ops, any float dtype) for the tests: the block, the whole forward
with injected Dropout2d scales, and one train step (summed yolo_loss, gradients by autograd, Adam)."""
import torch
import torch.nn.functional as Fn

from oracle.yolo_oracle import yolo_loss

SLOPE = 0.2


def param_names(num_blocks=10):
    names = ["conv1.weight", "conv1.bias"]
    for k in range(num_blocks):
        names += [f"residual_blocks.{k}.{c}.weight" for c in ("pointwise_conv1", "depthwise_conv", "pointwise_conv2")]
    return names + ["out.weight", "out.bias"]


def param_shapes(filters, num_blocks=10, in_ch=3, stem_k=10, head_k=6):
    sh = {"conv1.weight": (filters, in_ch, stem_k, stem_k), "conv1.bias": (filters,),
          "out.weight": (5, filters, head_k, head_k), "out.bias": (5,)}
    for k in range(num_blocks):
        sh[f"residual_blocks.{k}.pointwise_conv1.weight"] = (filters, filters, 1, 1)
        sh[f"residual_blocks.{k}.depthwise_conv.weight"] = (filters, 1, 3, 3)
        sh[f"residual_blocks.{k}.pointwise_conv2.weight"] = (filters, filters, 1, 1)
    return sh


def block_parts(x, w1, wd, w2, scale=None, pool=False):
    """-> (a, b, e, out): the two post-activation intermediates, the pre-pool sum and the block output."""
    a = Fn.leaky_relu(Fn.conv2d(x, w1), SLOPE)
    b = Fn.leaky_relu(Fn.conv2d(a, wd, padding=1, groups=x.shape[1]), SLOPE)
    c = Fn.conv2d(b, w2)
    if scale is not None:
        c = c * scale[:, :, None, None]
    e = c + x
    return a, b, e, (Fn.max_pool2d(e, 2) if pool else e)


def forward(P, x, masks=None, num_blocks=10, pool_above=16, stem=(8, 2), head_pad=0):
    h = Fn.conv2d(x, P["conv1.weight"], P["conv1.bias"], stride=stem[0], padding=stem[1])
    for k in range(num_blocks):
        nm = f"residual_blocks.{k}."
        h = block_parts(h, P[nm + "pointwise_conv1.weight"], P[nm + "depthwise_conv.weight"], P[nm + "pointwise_conv2.weight"],
                        None if masks is None else masks[f"residual_blocks.{k}"], pool=h.shape[2] > pool_above)[3]
    if masks is not None:
        h = h * masks["head"][:, :, None, None]
    return torch.sigmoid(Fn.conv2d(h, P["out.weight"], P["out.bias"], padding=head_pad))


def train_step(P, x, y, masks, lr=1e-4, **kw):
    """-> (y_train, loss, grads, params after one Adam step from zero moments)."""
    Q = {n: p.clone().requires_grad_(True) for n, p in P.items()}
    y_train = forward(Q, x, masks, **kw)
    loss = 0
    for n in range(x.shape[0]):
        loss = loss + yolo_loss(y_train[n], y[n])
    names = list(Q)
    grads = dict(zip(names, torch.autograd.grad(loss, [Q[n] for n in names])))
    after = {}
    b1, b2, eps = 0.9, 0.999, 1e-8
    for n in names:
        g = grads[n]
        m, v = (1 - b1) * g, (1 - b2) * g * g
        after[n] = P[n] - lr * (m / (1 - b1)) / ((v / (1 - b2)).sqrt() + eps)
    return y_train.detach(), loss.detach(), grads, after
