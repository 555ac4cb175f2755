"""ops.row_mean (dc_row_mean_f32) against np.mean(x, axis=0): the image-level feature vector's reduction on the device.  The kernel adds
sequentially over the rows and divides once, as NumPy does, so every comparison is exact (np.array_equal / torch.equal, no tolerance);
cases with K >= 3 first show on the host that the two tempting substitutes -- multiplying by float32(1 / K) and a pairwise sum -- give
other bits on the same data, so a kernel in either order could not pass."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from image_captioning_amd import ops as o
    return o


def _x(shape, seed=0):
    return (3.0 * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def _pairwise(x):
    """Sum over axis 0 as a tree (the halves summed on their own, then added), float32 throughout."""
    if x.shape[0] == 1:
        return x[0]
    n = x.shape[0] // 2
    return _pairwise(x[:n]) + _pairwise(x[n:])


def _sequential(x):
    s = x[0].copy()
    for k in range(1, x.shape[0]):
        s = s + x[k]
    return s


def _assert_orders_differ(x):
    K = x.shape[0]
    want = np.mean(x, axis=0)
    assert want.dtype == np.float32
    assert np.array_equal(want, _sequential(x) / np.float32(K)), "np.mean no longer adds sequentially and divides once"
    assert not np.array_equal(_sequential(x) * np.float32(1.0 / K), want), "this case cannot tell a multiplication by 1/K from the division"
    assert not np.array_equal(_pairwise(x) / np.float32(K), want), "this case cannot tell a pairwise sum from the sequential one"


@pytest.mark.parametrize("C_", [4, 260, 12544])
@pytest.mark.parametrize("K", [1, 2, 3, 7, 1000])
def test_row_mean_equals_numpy(ops, K, C_):
    x = _x((K, C_), seed=K * 100003 + C_)
    if K >= 3 and C_ > 4:
        _assert_orders_differ(x)
    elif K >= 3:                                  # four columns alone need not separate the orders: the wider case of this K does
        _assert_orders_differ(_x((K, 260), seed=K * 100003 + 260))
    got = ops.row_mean(torch.tensor(x, device="cuda"))
    assert got.dtype == torch.float32 and tuple(got.shape) == (C_,)
    assert np.array_equal(got.cpu().numpy(), np.mean(x, axis=0))


def test_row_mean_batched(ops):
    x = _x((3, 37, 260), seed=5)
    for b in range(3):
        _assert_orders_differ(x[b])
    got = ops.row_mean(torch.tensor(x, device="cuda"))
    assert tuple(got.shape) == (3, 260)
    assert np.array_equal(got.cpu().numpy(), np.mean(x, axis=1))
    # blocks cut out of a longer one: a batch stride that is not K * C (what generate_captions(image_level=True) passes)
    got = ops.row_mean(torch.tensor(x, device="cuda")[:, :20])
    assert np.array_equal(got.cpu().numpy(), np.mean(x[:, :20], axis=1))


def test_row_mean_row_stride_larger_than_c(ops):
    big = _x((37, 300), seed=6)
    for C_ in (260, 263):                         # 300 % 4 == 0: 16-byte loads, with a ragged last quad at 263
        x = big[:, :C_]
        _assert_orders_differ(np.ascontiguousarray(x))
        got = ops.row_mean(torch.tensor(big, device="cuda")[:, :C_])
        assert np.array_equal(got.cpu().numpy(), np.mean(x, axis=0))


def test_row_mean_scalar_path(ops):
    """A base pointer 4 bytes off a 16-byte boundary and C = 263: no row can be read 16 bytes at a time."""
    K, C_ = 37, 263
    x = _x((K, C_), seed=7)
    _assert_orders_differ(x)
    flat = torch.zeros(K * C_ + 1, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    xs = flat[1:].view(K, C_)
    xs.copy_(torch.tensor(x))
    assert xs.data_ptr() % 16 == 4
    assert np.array_equal(ops.row_mean(xs).cpu().numpy(), np.mean(x, axis=0))
    # the same data on the 16-byte path must give the same bits
    assert torch.equal(ops.row_mean(xs), ops.row_mean(torch.tensor(x, device="cuda")))


@pytest.mark.parametrize("path", ["vector", "scalar"])
@pytest.mark.parametrize("C_", [68, 64])
@pytest.mark.parametrize("K", [127, 128, 129, 256, 257])
def test_row_mean_tile_edges(ops, K, C_, path):
    """The double-buffered tile is 128 rows and the next one is fetched while t0 + 128 < K: one row short of a tile, a whole tile
    (nothing to prefetch), one row into a second tile, two whole tiles, one row into a third.  C = 64 is one block of columns, 68 a
    second block with one live quad.  scalar: the base 4 bytes past a 16-byte boundary, as in test_row_mean_scalar_path."""
    x = _x((K, C_), seed=K * 1009 + C_)
    want = _sequential(x) / np.float32(K)
    # what these cases are for is the order of the sum across tiles, which 64 columns always show; the division (multiplying by 1 / 128
    # or 1 / 256 IS dividing, and 1 / 257 differs in a column of a hundred) is told apart on the wider cases above
    assert not np.array_equal(_pairwise(x) / np.float32(K), want), "this case cannot tell a pairwise sum from the sequential one"
    assert np.array_equal(want, np.mean(x, axis=0))
    if path == "vector":
        xs = torch.tensor(x, device="cuda")
        assert xs.data_ptr() % 16 == 0
    else:
        flat = torch.zeros(K * C_ + 1, dtype=torch.float32, device="cuda")
        assert flat.data_ptr() % 16 == 0
        xs = flat[1:].view(K, C_)
        xs.copy_(torch.tensor(x))
        assert xs.data_ptr() % 16 == 4
    got = ops.row_mean(xs).cpu().numpy()
    assert got.shape == (C_,) and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_row_mean_production_size_and_out_reuse(ops):
    x = _x((1000, 12544), seed=8)                 # the RoIAlign block of one image: 50 MB, one launch
    _assert_orders_differ(x[:, :260])
    xd = torch.tensor(x, device="cuda")
    out = torch.full((12544,), 7.0, dtype=torch.float32, device="cuda")
    ptr = out.data_ptr()
    got = ops.row_mean(xd, out=out)
    assert got is out and out.data_ptr() == ptr
    want = np.mean(x, axis=0)
    assert np.array_equal(out.cpu().numpy(), want)
    # as the [1000,7,7,256] block itself
    assert np.array_equal(want, np.mean(x.reshape(1000, 7, 7, 256), axis=0).flatten())


def test_row_mean_refusals_write_nothing(ops):
    from image_captioning_amd import _lib
    lib = _lib.load()
    x = torch.ones((4, 8), dtype=torch.float32, device="cuda")
    out = torch.full((8,), 5.0, dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
    for B, K, C_, a, o in ((1, 0, 8, px, po), (1, 4, 0, px, po), (0, 4, 8, px, po), (1, -1, 8, px, po), (1, 4, 8, None, po), (1, 4, 8, px, None)):
        assert lib.dc_row_mean_f32(a, B, K, C_, 8, 0, o, 8, stream) == _lib.EINVAL, (B, K, C_)
    assert lib.dc_row_mean_f32(px, 1, 4, 8, 4, 0, po, 8, stream) == _lib.EINVAL          # a row stride below C
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 5.0))
    with pytest.raises(_lib.DcapError, match="code -1"):
        ops.row_mean(torch.empty((0, 8), dtype=torch.float32, device="cuda"), out=out)
    with pytest.raises(_lib.DcapError, match="code -1"):
        ops.row_mean(torch.empty((4, 0), dtype=torch.float32, device="cuda"))
    with pytest.raises(_lib.DcapError):
        ops.row_mean(torch.ones((8,), dtype=torch.float32, device="cuda"))
    assert torch.equal(out, torch.full_like(out, 5.0))
    assert np.array_equal(ops.row_mean(x, out=out).cpu().numpy(), np.ones(8, np.float32))
