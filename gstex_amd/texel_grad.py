"""The texel gradient's buffers, zero flags and routing (DESIGN.md "The texel gradient's life cycle"): one owner for
the state GStexTrainer's renders, gstex_amd.fused's backward and gstex_amd.dist.GradSync share.  Plain Python over
torch tensors (no HIP call): tests/test_texel_grad.py walks it on CPU tensors."""
import torch


class TexelGrad:
    def __init__(self):
        self._sink = None  # what the next differentiable render accumulates into (None: autograd owns the gradient)
        self._other = None  # own()'s second buffer: the raster backward zeroes it, the next step accumulates into it
        self._sink_zeroed = self._other_zeroed = False  # known to hold no gradient
        self._first = True  # no differentiable render since the last step / reset
        self._on_ready = self._route = self._param = None

    def own(self, param: torch.Tensor, double_buffer: bool):
        """A persistent gradient buffer for `param` (and a second one when double_buffer, unless a route is attached:
        it would never be used), both zero, the first one as param.grad."""
        self._param = param
        self._sink = param.grad = torch.zeros_like(param)
        self._other = torch.zeros_like(param) if double_buffer and self._route is None else None
        self._sink_zeroed, self._other_zeroed = True, self._other is not None

    def attach(self, sink: torch.Tensor, on_ready, route):
        """GradSync's hand-over: its flat buffer's tail slice as the sink, on_ready() once a backward's texel gradient
        is enqueued, route(first) -> (sink, zero_sink, on_ready) per differentiable render.  Drops the second buffer."""
        self._sink, self._on_ready, self._route = sink, on_ready, route
        self._other, self._other_zeroed = None, False

    @property
    def sink(self):
        return self._sink

    @property
    def routed(self) -> bool:
        """Whether a route is attached (GradSync owns the sink)."""
        return self._route is not None

    @property
    def double_buffered(self) -> bool:
        return self._other is not None

    def target(self, fused: bool):
        """(sink, zero_sink, first, on_grad, zero_next) of the render about to be enqueued: where its backward
        accumulates, whether its forward's grid zeroes that, whether it is the step's first differentiable render,
        what to call once its backward is enqueued, and the buffer its backward's grid zeroes (fused render only)."""
        first = self._first
        if self._route is not None and torch.is_grad_enabled():
            sink, zero_sink, on_grad = self._route(first)
        else:
            sink, zero_sink, on_grad = self._sink, first, self._on_ready
        zero_next = None
        if fused and self.double_buffered:
            zero_sink = first and not self._sink_zeroed
            zero_next = None if self._other_zeroed else self._other
        return sink, zero_sink, first, on_grad, zero_next

    def rendered(self):
        """A differentiable forward has been enqueued: later renders of the step accumulate on top."""
        self._first = self._sink_zeroed = False

    def zeroed_by_backward(self, buf: torch.Tensor, sink: torch.Tensor) -> bool:
        """Whether the backward of a node rendered into `sink` may zero `buf` (target()'s zero_next at its forward):
        only while `buf` is still the second buffer (no step, rechart or attach since).  Then it counts as zero."""
        ok = buf is self._other and buf.data_ptr() != sink.data_ptr()
        if ok:
            self._other_zeroed = True
        return ok

    def reset(self):
        """Discard what the sink holds: the next differentiable render is the step's first again."""
        self._first = True

    def stepped(self):
        """An optimizer step: -> the buffer its (deferred) texel update reads.  Double-buffered, the buffers swap: the
        next step accumulates into the other one while that update is pending."""
        self._first = True
        buf = self._sink
        if self.double_buffered:
            self._sink, self._other = self._other, buf
            self._sink_zeroed, self._other_zeroed = self._other_zeroed, False
            self._param.grad = self._sink
        return buf

    def state(self):
        """The flags and buffer addresses (tests: a call that must leave the training state alone)."""
        addr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return self._first, self._sink_zeroed, self._other_zeroed, addr(self._sink), addr(self._other)
