"""The evaluation kernels (csrc/eval_metrics.hip) against a torch CPU restatement of the reference's formulas
(conditional_flow_matching_multitask.py:326-343, conditional_flow_matching_multitask_multiclassloss.py:437-470):
exact integer counts, bit-equal dice_coef / iou, losses equal to the training loss kernels, the forward-only head + MSE
equal to head_fwd + mse_loss, and bit-identical repeats."""
import pytest
import torch

from stain2stain_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _logits(shape, seed, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(*shape, generator=g) * scale
    z[z.abs() < 1e-3] = 0.5                  # away from the sigmoid threshold's knife edge
    return z


def ref_binary(z, g):
    """The reference's metric block; z: CPU logits [B,1,H,W], g: integer 0/1 mask of the same shape."""
    pred = torch.sigmoid(z) > 0.5
    m = g.long()
    inter = (pred * m).sum()
    union = pred.sum() + m.sum()
    dice = (2.0 * inter + 1e-7) / (union + 1e-7)
    union = (pred | m).float().sum()
    iou = (inter + 1e-7) / (union + 1e-7)
    counts = [int(inter), int(pred.sum()), int(m.sum()), int(union)]
    return dice, iou, counts


def ref_multiclass(z, t, C, ignore_index):
    pred = torch.argmax(z, dim=1)
    mask = t.long()
    dices, ious, counts = [], [], []
    for c in range(C):
        pred_c, target_c = pred == c, mask == c
        counts.append([int((pred_c & target_c).sum()), int(pred_c.sum()), int(target_c.sum()),
                       int((pred_c | target_c).sum())])
        if c == ignore_index:
            continue
        inter = (pred_c & target_c).float().sum()
        union = pred_c.float().sum() + target_c.float().sum()
        dices.append((2.0 * inter + 1e-7) / (union + 1e-7))
        union = (pred_c | target_c).float().sum()
        ious.append((inter + 1e-7) / (union + 1e-7))
    return torch.stack(dices).mean(), torch.stack(ious).mean(), torch.tensor(counts).T


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-12)


BINARY_SHAPES = [(1, 7, 9), (2, 33, 17), (4, 64, 64), (8, 512, 512)]


@pytest.mark.parametrize("shape", BINARY_SHAPES)
@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_binary_counts_metrics_losses(shape, kind):
    B, H, W = shape
    z = _logits((B, 1, H, W), seed=B * 1000 + H)
    if kind == "random":
        m = (torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(H)) < 0.3).long()
    elif kind == "zeros":
        m = torch.zeros(B, 1, H, W, dtype=torch.long)
    else:
        m = torch.ones(B, 1, H, W, dtype=torch.long)
    dice, iou, counts = ref_binary(z, m)
    zg, mg = z.to(DEV), m.float().to(DEV)
    out, cnt = ops.seg_eval_binary(zg, mg)
    assert cnt.cpu().tolist() == counts
    assert out[3].cpu().item() == dice.item() and out[4].cpu().item() == iou.item()
    loss, _ = ops.seg_loss(zg, mg, want_grad=False)
    for i in range(3):
        assert _rel(out[i], loss[i]) < 1e-6, (i, float(out[i]), float(loss[i]))
    out2, cnt2 = ops.seg_eval_binary(zg, mg)
    assert torch.equal(out, out2) and torch.equal(cnt, cnt2)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bool])
def test_binary_mask_dtypes(dtype):
    z = _logits((2, 1, 31, 45), seed=5)
    m = torch.rand(2, 1, 31, 45, generator=torch.Generator().manual_seed(6)) < 0.5
    ref, ref_c = ops.seg_eval_binary(z.to(DEV), m.float().to(DEV))
    out, cnt = ops.seg_eval_binary(z.to(DEV), m.to(dtype).to(DEV))
    assert torch.equal(out, ref) and torch.equal(cnt, ref_c)
    out3, _ = ops.seg_eval_binary(z.to(DEV), m.to(dtype)[:, 0].to(DEV))        # [B,H,W] mask
    assert torch.equal(out3, ref)


def test_binary_rejects_bad_operands():
    z = torch.zeros(2, 1, 8, 8, device=DEV)
    with pytest.raises(RuntimeError):
        ops.seg_eval_binary(z, torch.zeros(2, 1, 8, 9, device=DEV))
    with pytest.raises(RuntimeError):
        ops.seg_eval_binary(torch.zeros(2, 2, 8, 8, device=DEV), torch.zeros(2, 2, 8, 8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.seg_eval_binary(z.double(), torch.zeros(2, 1, 8, 8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.seg_eval_binary(z.cpu(), torch.zeros(2, 1, 8, 8))


def _mc_case(B, C, H, W, seed, ties=True, absent=None):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, H, W, generator=g) * 2
    if ties:        # exact ties between classes 0 and 1 on every third row: torch.argmax takes the first index
        z[:, 1, ::3] = z[:, 0, ::3]
    t = torch.randint(0, C, (B, H, W), generator=g)
    if absent is not None:      # a class neither predicted nor present: its Dice and IoU are 1 by the 1e-7 terms
        t[t == absent] = (absent + 1) % C
        z[:, absent] = z.min() - 10.0
    return z, t


def _check_mc(z, t, C, ignore_index):
    dice, iou, counts = ref_multiclass(z, t, C, ignore_index)
    zg, tg = z.to(DEV), t.to(DEV)
    out, cnt = ops.seg_eval_multiclass(zg, tg, ignore_index)
    assert torch.equal(cnt.cpu(), counts)
    if C - (1 if 0 <= ignore_index < C else 0) <= 7:
        assert out[3].cpu().item() == dice.item() and out[4].cpu().item() == iou.item()
    else:       # torch's CPU sum of 8 fp32 terms runs in a host-dependent order: one ulp
        assert abs(out[3].cpu().item() - dice.item()) <= 2e-7 and abs(out[4].cpu().item() - iou.item()) <= 2e-7
    loss, _ = ops.seg_loss_multiclass(zg, tg, ignore_index, want_grad=False, validate=False)
    for i in range(3):
        assert _rel(out[i], loss[i]) < 1e-6, (i, float(out[i]), float(loss[i]))
    out2, cnt2 = ops.seg_eval_multiclass(zg, tg, ignore_index)
    assert torch.equal(out, out2) and torch.equal(cnt, cnt2)
    return out, cnt


@pytest.mark.parametrize("C", [2, 3, 4, 5, 6, 7, 8])
def test_multiclass_all_widths(C):
    z, t = _mc_case(2, C, 33, 17, seed=C)
    _check_mc(z, t, C, -100)


@pytest.mark.parametrize("C", [2, 5, 8])
def test_multiclass_production_size(C):
    z, t = _mc_case(8, C, 512, 512, seed=100 + C)
    _check_mc(z, t, C, -100)


def test_multiclass_first_index_wins_ties():
    z = torch.zeros(1, 4, 3, 5)
    z[:, 2] = 1.0
    z[:, 3] = 1.0                    # classes 2 and 3 tie everywhere: every pixel predicts 2
    t = torch.full((1, 3, 5), 3, dtype=torch.long)
    out, cnt = _check_mc(z, t, 4, -100)
    assert cnt[1, 2].item() == 15 and cnt[1, 3].item() == 0


@pytest.mark.parametrize("ignore_index", [-100, 0, 2, 4])
def test_multiclass_ignore_index(ignore_index):
    z, t = _mc_case(3, 5, 40, 24, seed=11 + ignore_index)
    out, cnt = _check_mc(z, t, 5, ignore_index)
    if 0 <= ignore_index < 5:        # P_c still counts the ignored pixels
        pred = torch.argmax(z, 1)
        assert cnt[1].sum().item() == pred.numel()


def test_multiclass_empty_class():
    z, t = _mc_case(2, 4, 16, 20, seed=3, absent=1)
    out, cnt = _check_mc(z, t, 4, -100)
    assert cnt[:, 1].tolist() == [0, 0, 0, 0]


def test_multiclass_b1_odd():
    z, t = _mc_case(1, 3, 9, 13, seed=4)
    _check_mc(z, t, 3, -100)
    _check_mc(z, t, 3, 1)


def test_multiclass_rejects_bad_operands():
    with pytest.raises(RuntimeError):
        ops.seg_eval_multiclass(torch.zeros(1, 9, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.long, device=DEV))
    with pytest.raises(RuntimeError):
        ops.seg_eval_multiclass(torch.zeros(1, 1, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.long, device=DEV))
    with pytest.raises(RuntimeError):
        ops.seg_eval_multiclass(torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 4, 5, dtype=torch.long, device=DEV))
    with pytest.raises(RuntimeError):
        ops.seg_eval_multiclass(torch.zeros(1, 3, 4, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV))


def test_multiclass_target_layouts():
    z, t = _mc_case(2, 3, 10, 12, seed=9)
    ref, rc = ops.seg_eval_multiclass(z.to(DEV), t.to(DEV))
    for tt in (t[:, None], t.to(torch.int32), t.to(torch.uint8)):
        out, cnt = ops.seg_eval_multiclass(z.to(DEV), tt.to(DEV))
        assert torch.equal(out, ref) and torch.equal(cnt, rc)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-6), (torch.bfloat16, 4e-3)])
@pytest.mark.parametrize("B,H,W,C,cout", [(2, 16, 24, 64, 3), (1, 9, 7, 24, 5), (3, 8, 8, 8, 1), (2, 32, 32, 128, 8),
                                          (16, 256, 256, 64, 3)])
def test_head_mse_eval_matches_head_and_mse(dtype, tol, B, H, W, C, cout):
    g = torch.Generator().manual_seed(C * 7 + cout)
    x = (torch.randn(B, H, W, C, generator=g)).to(dtype).to(DEV)
    w = (torch.randn(cout, C, 1, 1, generator=g) / C ** 0.5).to(DEV)
    b = torch.randn(cout, generator=g).to(DEV)
    u = torch.randn(B, cout, H, W, generator=g).to(DEV)
    v = ops.head_fwd(x, w, b)
    ref, _ = ops.mse_loss(v, u, want_grad=False) if v.numel() % 4 == 0 else (((v - u) ** 2).double().mean(), None)
    loss = ops.head_mse_eval(x, w, b, u)
    assert _rel(loss, ref) < tol, (float(loss), float(ref))
    assert torch.equal(loss, ops.head_mse_eval(x, w, b, u))
    assert _rel(ops.head_mse_eval(x, w, None, u), ((ops.head_fwd(x, w, None) - u) ** 2).double().mean()) < max(tol, 1e-5)


def test_head_mse_eval_channel_slice():
    g = torch.Generator().manual_seed(1)
    big = torch.randn(2, 12, 10, 80, generator=g).to(DEV)
    x = big[..., :64]                             # pixel stride 80
    w = torch.randn(3, 64, generator=g).to(DEV) / 8
    u = torch.randn(2, 3, 12, 10, generator=g).to(DEV)
    ref = ((ops.head_fwd(x.contiguous(), w, None) - u) ** 2).double().mean()
    assert _rel(ops.head_mse_eval(x, w, None, u), ref) < 1e-6


def test_head_mse_eval_rejects_bad_operands():
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    with pytest.raises(RuntimeError):
        ops.head_mse_eval(x, torch.zeros(9, 64, device=DEV), None, torch.zeros(1, 9, 4, 4, device=DEV))
    with pytest.raises(RuntimeError):
        ops.head_mse_eval(x, torch.zeros(3, 64, device=DEV), None, torch.zeros(1, 3, 4, 5, device=DEV))
    with pytest.raises(RuntimeError):
        ops.head_mse_eval(torch.zeros(1, 4, 4, 12, device=DEV), torch.zeros(3, 12, device=DEV), None,
                          torch.zeros(1, 3, 4, 4, device=DEV))
