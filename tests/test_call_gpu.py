"""_call on the device: the stream handle every launch gets is torch's current stream, and a launch through
``call`` lands on it."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    return torch.device("cuda:0")


def test_stream_handle_is_the_current_stream():
    from quantizationawarethzdoe_amd import _call
    dev = _dev()

    def handle():  # c_void_p(0).value is None: the default stream's handle
        return _call._stream_handle().value or 0

    with torch.cuda.device(dev):
        assert handle() == torch.cuda.current_stream().cuda_stream
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            assert handle() == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        assert handle() == torch.cuda.current_stream().cuda_stream


def test_call_launches_on_the_side_stream_and_raises_thz_error():
    from quantizationawarethzdoe_amd import _call, _lib
    dev = _dev()
    x = torch.randn(1, 1, 4, 4, dtype=torch.complex64, device=dev)
    out = torch.empty_like(x)
    d = _lib.ApertureDesc(BC=1, H=4, W=4, kind=_lib.APERTURE_CIRC, dx=1e-3, dy=1e-3, radius=10.0)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _call.call(_lib.lib().thz_aperture, d, x, out, device=dev)
    side.synchronize()  # the side stream alone: the launch was enqueued on it
    assert torch.equal(out, x)  # a radius beyond the grid: the mask is 1 everywhere
    with pytest.raises(_lib.ThzError) as e:
        _call.call(_lib.lib().thz_aperture, d, x, None, device=dev)
    assert e.value.code == _lib.THZ_E_ARG
