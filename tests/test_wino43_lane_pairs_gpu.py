"""The F(4x4, 3x3) kernels' lane and register pairings: the input transform's two half-patch lanes (l, l ^ 16), its column
pairs (0, 1) and the output step's channels (r, r + 1 share an accumulator's register pair), probed with inputs and weights
that move a single value through them.

The packed, ping-pong (pp) and precomputed-V (ppv) entry points must give the same bytes (the pre-pass behind ppv runs one
thread per whole patch: an independent statement of the transform) and stay within the bounds tests/test_conv_gpu.py sets
against conv2d: 5e-4 for the packed form, 1e-3 (fp64 reference) for pp and ppv.  Outputs go into sentinel-filled buffers,
so a store that is skipped or misplaced shows as well."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENTINEL = 3.0e30


def signed_bias(cout):
    """Neighbouring channels get biases of opposite sign, no two channels the same one: a bias (or a ReLU) that lands on
    the other channel of a pair changes the result."""
    c = torch.arange(cout, dtype=torch.float32)
    return (0.25 + c / cout) * (1.0 - 2.0 * (c % 2))


def run_all(x, wt, b, relu, wv):
    """-> (packed, pp, ppv) outputs on the CPU, each written into a sentinel-filled buffer."""
    from paddle3d_amd.ops import conv

    n, cin, h, w = x.shape
    cout = wt.shape[0]
    assert conv.winograd43_supported(cin, cout, h, w) and conv.winograd43_pp_supported(cin, cout, h, w)
    xc, bc = x.cuda(), None if b is None else b.cuda()
    ul = conv.pack_winograd43_lane_weight(wt.cuda())

    def buf():
        return torch.full((n, cout, h, w), SENTINEL, dtype=torch.float32, device="cuda")

    packed = conv.conv3x3_winograd43_bias_relu(xc, conv.pack_winograd43_weight(wt.cuda()), bc, cout, relu, out=buf(), w_valid=wv)
    pp = conv.conv3x3_winograd43_pp_bias_relu(xc, ul, bc, cout, relu, out=buf(), w_valid=wv)
    v = conv.winograd43_input_transform(xc, w_valid=wv)
    ppv = conv.conv3x3_winograd43_ppv_bias_relu(v, x.shape, ul, bc, cout, relu, out=buf(), w_valid=wv)
    return packed.cpu(), pp.cpu(), ppv.cpu()


def check_all(x, wt, b, relu, wv, what):
    ref = F.conv2d(x[..., :wv].double(), wt.double(), None if b is None else b.double(), padding=1)
    if relu:
        ref = torch.relu(ref)
    packed, pp, ppv = run_all(x, wt, b, relu, wv)
    wrong = []  # (every kernel is looked at before the test fails: which of them are off says where)
    for name, got, bound in (("packed", packed, 5e-4), ("pp", pp, 1e-3), ("ppv", ppv, 1e-3)):
        assert got.shape == x.shape[:1] + wt.shape[:1] + x.shape[2:], (what, name)
        if (got == SENTINEL).any():
            wrong.append((name, "elements left unwritten", int((got == SENTINEL).sum())))
        if not (got[..., wv:] == 0).all():
            wrong.append((name, "columns beyond w_valid not zero"))
        err = (got[..., :wv].double() - ref).abs()
        print(f"{what}: {name} max |error| {err.max().item():.3g} (bound {bound:g})")
        if not err.max().item() < bound:
            where = [tuple(int(v) for v in i) for i in (err >= bound).nonzero()[:4]]
            wrong.append((name, err.max().item(), int((err >= bound).sum()), where))
    if not torch.equal(pp, packed):
        wrong.append(("pp != packed", int((pp != packed).sum())))
    if not torch.equal(ppv, pp):
        wrong.append(("ppv != pp", int((ppv != pp).sum())))
    assert not wrong, (what, wrong)


def test_one_hot_inputs_at_every_position_of_a_tile_and_its_halo():
    """A single 1.0 per input plane: launch L puts it in row L, plane (image i, channel c) in column 64 i + c, and gives it
    to channel (c + 9 L) % 64 -- sixteen launches sweep every position of the four 8 x 64 workgroup tiles of a 16 x 128
    map (each tile's own 4 x 4 tiles, the halo rows and columns it shares with its neighbours, the image border), and
    every column meets every channel of a slot (9 L mod 8 runs through 0 .. 7 over a tile's eight rows).  Weights of order 1,
    different for every (cout, cin): a value that goes through the wrong lane, half or channel is off by about 1."""
    n, cin, cout, h, w = 2, 64, 64, 16, 128
    g = torch.Generator().manual_seed(43)
    wt = torch.randn(cout, cin, 3, 3, generator=g)
    b = signed_bias(cout)
    for L in range(h):
        x = torch.zeros(n, cin, h, w)
        for i in range(n):
            c = torch.arange(cin)
            x[i, (c + 9 * L) % cin, L, 64 * i + c] = 1.0
        check_all(x, wt, b, False, w, f"row {L}")


@pytest.mark.parametrize("relu", [True, False])
def test_one_hot_weights(relu):
    """A single tap of one (cout, cin) pair: that output channel is the input channel shifted by the tap (+ bias), every
    other channel its bias alone.  The nine taps, each on another pair of channels -- both halves of the output step's
    channel pairs (cout even and odd), several slots and channels within a slot -- on the general form (12 x 68, 66 valid
    columns: partial tiles, masked columns)."""
    n, cin, cout, h, w, wv = 1, 16, 128, 12, 68, 66
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, cin, h, w, generator=g)
    x[..., wv:] = 0
    b = signed_bias(cout)
    for t in range(9):
        co, ci = (29 * t + 2) % cout, (5 * t + 3) % cin
        wt = torch.zeros(cout, cin, 3, 3)
        wt[co, ci, t // 3, t % 3] = 1.0
        check_all(x, wt, b, relu, wv, f"tap {t} of ({co}, {ci})")


# batch 1 and 2; cin 8 (one slot), 16, 64; cout 64, 128; one whole workgroup tile, 2 x 2 of them, the general form
RANDOM_CASES = [(1, 8, 64, 8, 64, 64), (2, 16, 128, 8, 64, 64), (1, 64, 64, 8, 64, 64), (2, 8, 128, 16, 128, 128),
                (1, 16, 64, 16, 128, 128), (1, 64, 128, 16, 128, 128), (2, 8, 64, 12, 68, 66), (1, 16, 128, 12, 68, 66),
                (2, 64, 64, 12, 68, 66)]


@pytest.mark.parametrize("n,cin,cout,h,w,wv", RANDOM_CASES)
@pytest.mark.parametrize("relu", [True, False])
def test_seeded_random(n, cin, cout, h, w, wv, relu):
    g = torch.Generator().manual_seed(1000 * cin + cout + h)
    x = torch.randn(n, cin, h, w, generator=g)
    x[..., wv:] = 0
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    check_all(x, wt, signed_bias(cout), relu, wv, "random")
