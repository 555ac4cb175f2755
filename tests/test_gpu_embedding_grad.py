"""ops.embedding_grad (dc_embedding_grad_f32): the gradient of a trainable embedding table, exact against the same sums taken in
ascending row order in float32 (the kernel's fixed order), and within float32 rounding of the float64 scatter-add."""
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


def _want(dx, ids, V):
    out = np.zeros((V, dx.shape[1]), np.float32)
    for m, v in enumerate(ids):                       # ascending m, float32 adds: the kernel's order
        if 0 <= v < V:
            out[v] += dx[m]
    return out


@pytest.mark.parametrize("n,V,W", [(1, 4, 4), (37, 8, 33), (148, 52, 32), (300, 7, 260), (1000, 64, 256)])
def test_embedding_grad_is_exact(ops, n, V, W):
    rng = np.random.default_rng(n * 1000 + V)
    dx = rng.standard_normal((n, W)).astype(np.float32)
    ids = rng.integers(0, V, n).astype(np.int32)
    if n > 100:
        ids[ids == 3] = 2                             # word 3 never occurs: its row must come back as zeros
    out = torch.full((V, W), 9.0, dtype=torch.float32, device="cuda")
    got = ops.embedding_grad(torch.tensor(dx, device="cuda"), torch.tensor(ids, device="cuda"), out)
    assert got is out
    want = _want(dx, ids, V)
    assert np.array_equal(out.cpu().numpy(), want)
    if n > 100:
        assert np.all(want[3] == 0)
    w64 = np.zeros((V, W))
    np.add.at(w64, ids, dx.astype(np.float64))
    assert np.abs(want - w64).max() <= 1e-6 * max(1.0, np.abs(w64).max()) * np.sqrt(n)


def test_embedding_grad_strides_and_foreign_ids(ops):
    rng = np.random.default_rng(5)
    big = rng.standard_normal((50, 40)).astype(np.float32)
    ids = rng.integers(-2, 12, 50).astype(np.int32)            # ids outside [0, V) contribute nothing
    table = torch.full((10, 48), 9.0, dtype=torch.float32, device="cuda")
    ops.embedding_grad(torch.tensor(big, device="cuda")[:, :33], torch.tensor(ids, device="cuda"), table[:, :33])
    got = table.cpu().numpy()
    assert np.array_equal(got[:, :33], _want(big[:, :33], ids, 10)) and np.all(got[:, 33:] == 9.0)


def test_embedding_grad_refusals(ops):
    from image_captioning_amd import _lib
    dx = torch.ones((4, 8), dtype=torch.float32, device="cuda")
    ids = torch.zeros((4,), dtype=torch.int32, device="cuda")
    out = torch.full((3, 8), 5.0, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.DcapError):
        ops.embedding_grad(dx, ids[:3], out)
    with pytest.raises(_lib.DcapError):
        ops.embedding_grad(dx, ids, out[:, :4])
    with pytest.raises(_lib.DcapError):
        ops.embedding_grad(dx, ids.to(torch.int64), out)
    assert torch.equal(out, torch.full_like(out, 5.0))
