"""make_grid: the image grid of torchvision.utils.make_grid (padding, pad_value and nrow; no normalisation), for the
plotting rows of LatentDiffusion.log_images without a torchvision dependency."""
import math

import torch


def make_grid(tensor, nrow=8, padding=2, pad_value=0.0):
    """[N, C, H, W] (or a list of [C, H, W]) -> [C', (H + p) * ymaps + p, (W + p) * xmaps + p] with xmaps = min(nrow, N)
    images per row, ymaps = ceil(N / xmaps) rows, `padding` pixels of `pad_value` around every image; one channel is
    repeated to three, and a single image is returned as it is."""
    if isinstance(tensor, (list, tuple)):
        tensor = torch.stack(list(tensor), dim=0)
    if tensor.dim() == 2:
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 3:
        if tensor.size(0) == 1:
            tensor = torch.cat((tensor, tensor, tensor), 0)
        tensor = tensor.unsqueeze(0)
    if tensor.dim() == 4 and tensor.size(1) == 1:
        tensor = torch.cat((tensor, tensor, tensor), 1)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    n = tensor.size(0)
    xmaps = min(nrow, n)
    ymaps = int(math.ceil(float(n) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((tensor.size(1), height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(
                2, x * width + padding, width - padding).copy_(tensor[k])
            k += 1
    return grid
