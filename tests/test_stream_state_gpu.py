"""The device library's per-stream state (csrc/lib_state.hip: scratch block, stream-K arrival counters, tickets; csrc/norm.hip:
the GroupNorm statistics buffers) under callers on two streams at once, in the steady state, and under capture.

Every comparison is between a call made on one of two busy streams and the SAME call made alone on the default stream, within
the dense-convolution tolerance of the active math mode (tests/test_ops_gpu.py test_conv2d_matches_torch, through the helper
tests/test_conv_geometry_gpu.py keeps for it).  The 16-stream limit of the tables is tested on the host
(tests/test_per_stream_host.py): filling them here would fill them for every later test of the process."""
import pytest
import torch

from lsnet_amd import _lib
from tests.test_conv_geometry_gpu import _tol
from tests.test_ops_gpu import _dev, _err

pytestmark = pytest.mark.gpu

_CL = torch.channels_last
LSN_ERR_RUNTIME = -3
# B, C, H, W, Co of the two 3x3 convolutions (csrc/conv_route.h; both are rows of tests/test_conv_route_host.py):
#   Z_SPLIT: one 128 x 64 tile under 72 chunks -> 9 blockIdx.z splits + the reduce launch (data gradient: 2 splits)
#   STREAM_K: 130 tiles of 64 x 128 under 18 chunks -> 512 stream-K pieces over scratch + arrival counters (data gradient: 65
#             tiles, 4 blockIdx.z splits)
Z_SPLIT = (1, 256, 8, 8, 64)
STREAM_K = (2, 64, 65, 64, 128)


@pytest.fixture(scope='module')
def streams():
    return torch.cuda.Stream(), torch.cuda.Stream()


# ---- the work: inputs(seed) on the default stream, then two steps whose launches the streams interleave ----
class ConvWork:
    def __init__(self, shape):
        self.shape = shape

    def inputs(self, seed):
        B, C, H, W, Co = self.shape
        g = torch.Generator(device='cpu').manual_seed(seed)
        x = torch.randn(B, C, H, W, generator=g).to(_dev()).contiguous(memory_format=_CL).requires_grad_()
        w = (torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5).to(_dev()).contiguous(memory_format=_CL).requires_grad_()
        b = torch.randn(Co, generator=g).to(_dev()).requires_grad_()
        go = torch.randn(B, Co, H, W, generator=g).to(_dev()).contiguous(memory_format=_CL)
        return x, w, b, go

    def forward(self, inp):
        from lsnet_amd.ops.conv import conv2d
        x, w, b, _ = inp
        return conv2d(x, w, b, 1, 1, 1)

    def backward(self, inp, y):
        x, w, b, go = inp
        return [y.detach()] + list(torch.autograd.grad(y, [x, w, b], go))


class NormWork:
    def inputs(self, seed):
        from lsnet_amd.ops.group_norm import GroupNorm
        g = torch.Generator(device='cpu').manual_seed(seed)
        gn = GroupNorm(8, 32).to(_dev())
        with torch.no_grad():
            gn.weight.copy_(torch.randn(32, generator=g))
            gn.bias.copy_(torch.randn(32, generator=g))
        x = (torch.randn(2, 32, 16, 16, generator=g) * 2 + 0.5).to(_dev()).contiguous(memory_format=_CL).requires_grad_()
        go = torch.randn(2, 32, 16, 16, generator=g).to(_dev()).contiguous(memory_format=_CL)
        return gn, x, go

    def forward(self, inp):
        gn, x, _ = inp
        return gn.forward_multi([x], relu=False)[0]

    def backward(self, inp, y):
        gn, x, go = inp
        return [y.detach()] + list(torch.autograd.grad(y, [x, gn.weight, gn.bias], go))


class FocalWork:
    B, LEVELS, C = 2, [100, 40, 10], 80        # N = 2 x 150 = 300 rows

    def inputs(self, seed):
        g = torch.Generator(device='cpu').manual_seed(seed)
        N = self.B * sum(self.LEVELS)
        lg = (torch.randn(N, self.C, generator=g) * 4).to(_dev())
        tg = torch.randint(0, self.C + 1, (N,), generator=g).to(_dev())
        w = torch.rand(N, generator=g).to(_dev())
        return lg, tg, w

    def forward(self, inp):
        from lsnet_amd import ops
        lg, tg, w = inp
        return ops.sigmoid_focal_loss_sum(lg, tg, w, 2.0, 0.25)

    def backward(self, inp, s):
        from lsnet_amd.ops.focal import sigmoid_focal_loss_level_sums
        lg, tg, w = inp
        return [s, sigmoid_focal_loss_level_sums(lg, tg, w, self.B, self.LEVELS, 2.0, 0.25)]


WORK = {'z_split': ConvWork(Z_SPLIT), 'stream_k': ConvWork(STREAM_K), 'group_norm': NormWork(), 'focal': FocalWork()}
_cache = {}


def _case(name):
    """(inputs of stream 0, inputs of stream 1, their results alone on the default stream): made once, never modified"""
    if name not in _cache:
        work = WORK[name]
        inps = [work.inputs(100 + 7 * i + 1000 * sorted(WORK).index(name)) for i in range(2)]
        alone = []
        for inp in inps:
            torch.cuda.synchronize()
            alone.append([t.clone() for t in work.backward(inp, work.forward(inp))])
            torch.cuda.synchronize()
        _cache[name] = (inps, alone)
    return _cache[name]


def _on_two_streams(name, streams):
    """both streams' calls in flight together: forward on 0, forward on 1, backward on 0, backward on 1, no wait in between"""
    work = WORK[name]
    inps, _ = _case(name)
    torch.cuda.synchronize()
    mid, out = [None, None], [None, None]
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            mid[i] = work.forward(inps[i])
    for i, s in enumerate(streams):
        with torch.cuda.stream(s):
            out[i] = work.backward(inps[i], mid[i])
    torch.cuda.synchronize()
    return out


def _hold(name, got, alone):
    tol = _tol(_lib.get_math_mode())
    errs = [[_err(g.double(), r.double()) for g, r in zip(gs, rs)] for gs, rs in zip(got, alone)]
    print(f'STREAMS {name} tol {tol:.1e} ' + ' | '.join(' '.join(f'{e:.2e}' for e in es) for es in errs))
    for i, es in enumerate(errs):
        for k, e in enumerate(es):
            assert e < tol, (name, f'stream {i}', f'result {k}', e)


@pytest.mark.parametrize('name', ['z_split', 'stream_k'])
def test_two_streams_split_reductions(name, streams):
    """Forward, data gradient, weight and bias gradient of a convolution whose partial tiles go through the stream's scratch
    block -- the blockIdx.z split with its reduce launch, and stream-K pieces with their arrival counters -- on two streams at
    once with different inputs: each stream gets what the call gives alone."""
    inps, alone = _case(name)
    assert not torch.equal(inps[0][0], inps[1][0]) and not torch.equal(alone[0][0], alone[1][0])
    _hold(name, _on_two_streams(name, streams), alone)


@pytest.mark.parametrize('name', ['group_norm', 'focal'])
def test_two_streams_tickets_and_sums(name, streams):
    """GroupNorm forward + backward (per-stream statistics buffers, the image sums' ticket) and the two focal sums (1024 partial
    sums in the stream's scratch block, their own ticket) on two streams at once: no stream sees the other's partial sums."""
    inps, alone = _case(name)
    assert not torch.equal(alone[0][0], alone[1][0])
    _hold(name, _on_two_streams(name, streams), alone)


def test_steady_state_allocates_and_waits_for_nothing(streams):
    """After one pass of every case on both streams the library asks the HIP runtime for nothing more: a second pass leaves
    lsn_scratch_stats where it was -- no allocation, no blocking synchronisation."""
    for name in WORK:
        _on_two_streams(name, streams)
    before = _lib.scratch_stats()
    got = {name: _on_two_streams(name, streams) for name in WORK}
    assert _lib.scratch_stats() == before, (before, _lib.scratch_stats())
    for name in WORK:
        _hold(name, got[name], _case(name)[1])


def test_first_call_under_capture_is_refused_on_the_host():
    """A stream the library has never seen, being captured: the first call that needs scratch returns LSN_ERR_RUNTIME with the
    library's advice before it launches or allocates anything, and the capture goes on undisturbed."""
    from lsnet_amd.ops.conv import weight_image
    lib = _lib.load()
    B, C, H, W, Co = Z_SPLIT
    x, w, b, _ = _case('z_split')[0][0]
    img = weight_image(w, 0)                       # built eagerly, on the default stream
    out = torch.empty((B, Co, H, W), device=x.device, memory_format=_CL)
    marker = torch.zeros(4, device=x.device)
    lv = (_lib.ConvLevel * 1)()
    lv[0].x, lv[0].out, lv[0].B, lv[0].H, lv[0].W = _lib.ptr(x), _lib.ptr(out), B, H, W
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    before = _lib.scratch_stats()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        marker.add_(1)                             # (so that the discarded graph is not an empty one)
        rc = lib.lsn_conv2d_forward_prepared(1, lv, _lib.ptr(img), _lib.ptr(b), C, C, Co, 3, 3, 1, 1, 1, 0, s.cuda_stream)
        msg = lib.lsn_last_error().decode()
    del graph
    torch.cuda.synchronize()
    assert rc == LSN_ERR_RUNTIME, (rc, msg)
    assert 'run the step eagerly once before capturing' in msg, msg
    assert _lib.scratch_stats() == before
    assert float(marker.sum()) == 0.0              # captured, never replayed
