"""The cases tests/test_select.py and tests/test_gpu_select.py share: the standard chart list, the standard masks, the
arange-distinct sources with sentinel capacity rows and the plain-loop restatement of the selection."""
import torch

# (h, w) per splat, cycled: zero-texel charts with and without non-zero dims, one-texel charts, a 272-texel chart
# (more than a 256-thread workgroup) and a 1600-texel chart (more than the texel gather's 1024-texel run)
PATTERN = [(0, 0), (1, 1), (1, 1), (3, 5), (0, 4), (7, 1), (16, 17), (1, 1), (40, 40), (2, 2)]
PATTERN_TEXELS = 1901
SENTINEL = -12345.0
CAPACITY_ROWS = 100
GUARD_ROWS = 64


def chart_list(n=600, reverse=False, start=0):
    """texture_dims (n, 3) int32 of the pattern cycled from `start`, offsets the exclusive sum of h * w (reverse: the
    blocks laid out in the opposite order, splat 0's block last) -> (dims, T)."""
    hw = torch.tensor([PATTERN[(start + i) % len(PATTERN)] for i in range(n)], dtype=torch.int64)
    size = hw[:, 0] * hw[:, 1]
    end = torch.cumsum(size, 0)
    T = int(end[-1])
    off = (T - end) if reverse else (end - size)
    return torch.cat([hw, off[:, None]], 1).to(torch.int32), T


def sources(T, channels=3, count=3, sentinel=SENTINEL):
    """`count` texel tensors (T + CAPACITY_ROWS, channels): distinct integers per tensor (exact in fp32), the capacity
    rows filled with the sentinel."""
    out = []
    for k in range(count):
        t = torch.full((T + CAPACITY_ROWS, channels), sentinel, dtype=torch.float32)
        t[:T] = (torch.arange(T * channels, dtype=torch.float32) + float(k * 4_000_000 + 1)).view(T, channels)
        out.append(t)
    return out


def masks(dims):
    n = dims.shape[0]
    i = torch.arange(n)
    size = dims[:, 0].long() * dims[:, 1].long()
    g = torch.Generator().manual_seed(11)
    return {
        "all": torch.ones(n, dtype=torch.bool),
        "every_other": i % 2 == 0,
        "first": i == 0,
        "last": i == n - 1,
        "runs_37_23": i % 60 < 37,
        "bernoulli": torch.rand(n, generator=g) < 0.5,
        "zero_texel_only": size == 0,
        "no_1600": size != 1600,
    }


MASK_NAMES = ["all", "every_other", "first", "last", "runs_37_23", "bernoulli", "zero_texel_only", "no_1600"]


def loop_select(dims, keep, tensors):
    """The selection as a plain loop: per kept splat, slice its block and concatenate."""
    rows, blocks, off = [], [[] for _ in tensors], 0
    for i in range(dims.shape[0]):
        if not bool(keep[i]):
            continue
        h, w, o = (int(v) for v in dims[i])
        rows.append([h, w, off])
        for k, t in enumerate(tensors):
            blocks[k].append(t[o:o + h * w])
        off += h * w
    new_dims = torch.tensor(rows, dtype=torch.int32).reshape(-1, 3)
    new = [torch.cat(b) if b else t[:0] for b, t in zip(blocks, tensors)]
    return new_dims, new, off


def guarded_alloc(device, sentinel=SENTINEL):
    """An alloc callback for select_texture whose results are views of larger buffers with GUARD_ROWS sentinel rows
    behind them -> (alloc, buffers)."""
    buffers = {}

    def alloc(k, shape):
        buf = torch.full((shape[0] + GUARD_ROWS,) + tuple(shape[1:]), sentinel, dtype=torch.float32, device=device)
        buffers[k] = buf
        return buf[:shape[0]]
    return alloc, buffers
