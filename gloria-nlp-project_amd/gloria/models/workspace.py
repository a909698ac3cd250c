"""fp32 scratch of the kernels that reduce across rows (fused_ln: d-gamma / d-beta / bias partials; fused_linear: column
sums): one buffer per (device, stream), grown on demand, its size asked from the library once per shape."""

import torch

from .. import _native as N


def make_workspace(floats_symbol, floor):
    """-> workspace(dev, R, C): at least `floats_symbol`(R, C) floats for a launch on the current stream, or None when the
    library asks for none (a shape it does not take).  `floor`: the smallest buffer allocated."""
    sizes = {}          # (R, C) -> floats: one ctypes call per shape, not per launch (host time)
    buffers = {}        # (device index, stream) -> fp32 workspace: launches of one stream only (see fused_bn)

    def workspace(dev, R, C):
        n = sizes.get((R, C))
        if n is None:
            if len(sizes) >= 64:         # the packed text route changes R every step: the cache stays small
                sizes.clear()
            n = sizes[(R, C)] = int(getattr(N.lib(), floats_symbol)(R, C))
        if n == 0:
            return None
        if torch.cuda.is_current_stream_capturing():        # a graph keeps its own: the shared one may be replaced later
            return torch.empty(n, dtype=torch.float32, device=dev)
        key = (dev.index, N.stream())
        ws = buffers.get(key)
        if ws is None or ws.numel() < n:
            ws = buffers[key] = torch.empty(max(n, floor), dtype=torch.float32, device=dev)
        return ws

    return workspace
