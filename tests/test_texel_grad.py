"""gstex_amd.texel_grad.TexelGrad alone, on CPU tensors: the transitions of the texel gradient's buffers, zero flags
and routing that GStexTrainer, gstex_amd.fused and GradSync drive (tests/test_gpu_texel_grad.py pins the launches
they result in)."""
import torch

from gstex_amd.texel_grad import TexelGrad


def _addr(t):
    return None if t is None else t.data_ptr()


def test_transitions():
    p = torch.nn.Parameter(torch.randn(40, 3))
    tg = TexelGrad()
    assert tg.sink is None and not tg.double_buffered
    assert tg.target(False) == (None, True, True, None, None)  # (autograd owns the gradient: nothing to zero into)

    # 1. own: two zero buffers, the first one the parameter's gradient
    tg.own(p, double_buffer=True)
    a = tg.sink
    assert tg.double_buffered and p.grad is a and a.shape == p.shape and not a.any()
    first, a_zero, b_zero, sink_addr, b_addr = tg.state()
    assert (first, a_zero, b_zero, sink_addr) == (True, True, True, a.data_ptr()) and b_addr not in (None, sink_addr)

    # 2. the per-op render zeroes in its forward even though the buffer is known to be zero
    sink, zero_sink, first, on_grad, zero_next = tg.target(fused=False)
    assert sink is a and zero_sink is True and first is True and on_grad is None and zero_next is None
    assert tg.state() == (True, True, True, a.data_ptr(), b_addr)  # (target() itself changes nothing)

    # 3. rendered, stepped: the buffers swap, the update reads the old sink
    tg.rendered()
    assert tg.state() == (False, False, True, a.data_ptr(), b_addr)
    assert tg.target(False)[1:3] == (False, False)  # a second render of the step accumulates on top
    buf = tg.stepped()
    b = tg.sink
    assert buf is a and b is not a and b.data_ptr() == b_addr and p.grad is b
    assert tg.state() == (True, True, False, b.data_ptr(), a.data_ptr())

    # 4. the fused render: the sink is known to be zero, its backward zeroes the old one
    sink, zero_sink, first, on_grad, zero_next = tg.target(fused=True)
    assert sink is b and zero_sink is False and first is True and zero_next is a
    tg.rendered()

    # 6. a foreign tensor (a buffer of before a rechart) is not zeroed and changes no flag
    before = tg.state()
    assert tg.zeroed_by_backward(torch.zeros_like(p), b) is False and tg.state() == before
    assert tg.zeroed_by_backward(b, b) is False and tg.state() == before  # nor the node's own sink
    # 5. the old sink is
    assert tg.zeroed_by_backward(a, b) is True
    assert tg.state() == (False, False, True, b.data_ptr(), a.data_ptr())

    # 7. reset (a skipped step): the second render is a first one whose sink holds a gradient
    tg.reset()
    sink, zero_sink, first, on_grad, zero_next = tg.target(fused=True)
    assert sink is b and zero_sink is True and first is True and zero_next is None
    tg.rendered()
    # a step whose backward did not zero the other buffer (per-op render): the next forward zeroes its sink
    assert tg.stepped() is b and tg.sink is a
    assert tg.state() == (True, True, False, a.data_ptr(), b.data_ptr())
    tg.rendered()
    assert tg.stepped() is a
    assert tg.target(fused=True)[1:] == (True, True, None, a)
    # after a step, a buffer handed to an earlier backward is no longer the other one
    assert tg.zeroed_by_backward(b, a) is False

    # 8. attach: the second buffer goes, target() returns what the route returns
    flat = torch.zeros(200)
    tail, side = flat[64:184].view(40, 3), torch.zeros(40, 3)
    routed = []

    def ready():
        pass

    def route(first):
        routed.append(first)
        return (tail, first, ready) if first else (side, False, None)

    tg.attach(tail, ready, route)
    assert not tg.double_buffered and tg.sink is tail and tg.state()[2:] == (False, tail.data_ptr(), None)
    assert tg.target(fused=True) == (tail, True, True, ready, None)
    tg.rendered()
    assert tg.target(fused=False) == (side, False, False, None, None)
    assert routed == [True, False]
    assert tg.stepped() is tail and tg.sink is tail  # (nothing to swap)

    # 9. without grad enabled the route is not consulted
    with torch.no_grad():
        assert tg.target(fused=False) == (tail, True, True, ready, None)
    assert routed == [True, False]

    # a rechart that grows the store under a route: one fresh buffer until GradSync attaches its new slice
    q = torch.nn.Parameter(torch.randn(55, 3))
    tg.own(q, double_buffer=True)
    assert not tg.double_buffered and q.grad is tg.sink and tg.sink.shape == q.shape
