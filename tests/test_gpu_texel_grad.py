"""What the raster grids zero of the texel gradient, per training configuration (gstex_amd.texel_grad, DESIGN.md
"The texel gradient's life cycle"): the `zero_buf` arguments of every gstex_raster_fwd / gstex_raster_bwd launch of a
run of training steps, recorded at ops._launch.  The other trainer tests check that the configurations train alike;
this one pins the property the machinery exists for -- in the steady state no forward spends its grid zeroing the
texel-gradient buffer (120 MB at cfg3) -- and that a step's first render, and only it, zeroes where one must."""
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu
H = W = 96


class _Trace:
    """ops._launch wrapped by a recorder: (kernel, zero_buf address or 0) of the raster launches (the forward's
    zero_buf2, its partial sums, is not part of the check)."""

    def __init__(self, monkeypatch):
        from gstex_amd import ops

        self.calls = []
        inner = ops._launch

        def launch(name, *args):
            if name in ("gstex_raster_fwd", "gstex_raster_bwd"):
                self.calls.append((name[len("gstex_raster_"):], args[0]._obj.zero_buf or 0))
            return inner(name, *args)

        monkeypatch.setattr(ops, "_launch", launch)

    def take(self):
        """The launches recorded since the last take()."""
        out, self.calls = self.calls, []
        return out


def _setup(**kw):
    from gstex_amd.model import GStexTrainer
    from gstex_amd.scene import make_scene, sphere_view

    dev = torch.device("cuda", 0)
    tr = GStexTrainer(make_scene(3000, 60_000, seed=31), dev, start_step=3000, defer_texture=True, **kw)
    views = [sphere_view(i, H, W).to(dev) for i in range(2)]
    g = torch.Generator().manual_seed(11)
    gts = [torch.rand((H, W, 3), generator=g).to(dev) for _ in range(2)]
    return tr, lambda i=0: tr.forward_backward(views[i % 2], gts[i % 2])


def test_double_buffered_fused_step_zeroes_in_the_backward(monkeypatch):
    """defer_texture with the defaults (fused step, pair capacity): two buffers A and B; step k accumulates into one
    and its backward zeroes the other, so from the second step on no forward zeroes anything."""
    tr, fb = _setup()
    trace = _Trace(monkeypatch)
    assert tr.defer_texture and tr.fused_step and tr.pairs is not None and tr.texel_grad.double_buffered
    sinks = []
    for k in range(5):
        tr.zero_grad()
        s = tr.texture_grad_sink.data_ptr()
        sinks.append(s)
        assert tr._fused_ok(False, None) == (k > 0)  # (the first render sizes the pair capacity: the per-op path)
        fb(k)
        tr.optimizer_step()
        if k == 0:
            assert trace.take() == [("fwd", s), ("bwd", 0)]
        else:
            other = sinks[0] if s == sinks[1] else sinks[1]
            assert trace.take() == [("fwd", 0), ("bwd", other)], f"step {k + 1}"
    a, b = sinks[:2]
    assert a != b and sinks == [a, b, a, b, a]
    # a backward whose step is skipped: the next render re-zeroes the sink in its forward (the other buffer is
    # already zero)
    tr.zero_grad()
    s = tr.texture_grad_sink.data_ptr()
    other = a if s == b else b
    fb(0)
    assert trace.take() == [("fwd", 0), ("bwd", other)]
    tr.zero_grad()
    assert tr.texture_grad_sink.data_ptr() == s
    fb(1)
    assert trace.take() == [("fwd", s), ("bwd", 0)]
    tr.optimizer_step()
    # two renders of one step: the second accumulates on top, nothing left to zero
    tr.zero_grad()
    s = tr.texture_grad_sink.data_ptr()
    assert s == other
    fb(0)
    fb(1)
    assert trace.take() == [("fwd", 0), ("bwd", a if s == b else b), ("fwd", 0), ("bwd", 0)]
    tr.optimizer_step()
    tr.wait_texture()
    torch.cuda.synchronize()
    assert tr.skipped_steps == []


def test_per_op_step_zeroes_the_one_sink_in_the_first_forward(monkeypatch):
    """defer_texture, fused_step=False: one persistent sink, zeroed by each step's first raster forward."""
    tr, fb = _setup(fused_step=False)
    trace = _Trace(monkeypatch)
    assert not tr.texel_grad.double_buffered
    s = tr.texture_grad_sink.data_ptr()
    for k in range(3):
        tr.zero_grad()
        fb(k)
        if k == 1:
            fb(k + 1)  # a second render in the step
        tr.optimizer_step()
        assert tr.texture_grad_sink.data_ptr() == s
        assert trace.take() == [("fwd", s), ("bwd", 0)] + ([("fwd", 0), ("bwd", 0)] if k == 1 else [])
    tr.wait_texture()
    torch.cuda.synchronize()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_gradsync_step_zeroes_the_flat_buffers_tail_in_the_first_forward(monkeypatch):
    """defer_texture under GradSync (world 1 over RCCL): the sink is the flat buffer's tail slice, zeroed by each step's
    first raster forward (fused render or not); the trainer's second buffer is dropped."""
    import torch.distributed as dist

    from gstex_amd.dist import GradSync

    if not dist.is_initialized():
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_port()}", rank=0, world_size=1)
    try:
        tr, fb = _setup()
        sync = GradSync(tr, 1)
        trace = _Trace(monkeypatch)
        assert not tr.texel_grad.double_buffered
        tail = sync.flat[sync._tail_off:].data_ptr()
        for k in range(4):
            sync.zero()
            assert tr.texture_grad_sink.data_ptr() == tail
            assert tr._fused_ok(False, None) == (k > 0)
            fb(k)
            tr.optimizer_step(sync=sync)
            assert trace.take() == [("fwd", tail), ("bwd", 0)], f"step {k + 1}"
        tr.wait_texture()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
