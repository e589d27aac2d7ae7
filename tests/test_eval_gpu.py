"""GPU (-m gpu): unet_eval_confusion / unet_eval_maps and the evaluation loop built on them.

Counts are compared with integer equality: the kernel and what it is held against (the reference's
recorded accumulators in tests/golden/eval.npz, numpy restatements written here, and compositions
of torch's own argmax / F.interpolate / bincount on the same device logits) see identical fp32
logits and only compare them."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(
        name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


E = _load("eval_inputs")
CASE = {c[0]: c for c in E.CASES}


def case_tensors(name):
    _, seed, H, W, dims, classes = CASE[name]
    logits, target = E.make_case(seed, len(dims), H, W, classes)
    return logits, target, dims


@pytest.mark.parametrize("name", [c[0] for c in E.CASES])
def test_eval_confusion_equals_the_reference_counts(ua, golden, name):
    g = golden("eval")
    logits, target, dims = case_tensors(name)
    d = torch.tensor(dims, dtype=torch.int64).cuda()
    cm = ua.ops.eval_confusion(torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda(), d)
    assert cm.dtype == torch.int64 and tuple(cm.shape) == (len(dims), 3, 3)
    cm = cm.cpu().numpy()
    # the reference's accumulators, per image: intersections, TP + FN, TP + FP
    acc = np.diff(np.concatenate([np.zeros((1, 17)), g[f"acc_{name}"]]), axis=0)
    pred = logits.argmax(axis=1)
    for b in range(len(dims)):
        assert np.array_equal(np.diagonal(cm[b]), acc[b, 0:3]), (name, b)
        assert np.array_equal(cm[b].sum(axis=1), acc[b, 6:9] + acc[b, 12:15]), (name, b)
        assert np.array_equal(cm[b].sum(axis=0), acc[b, 6:9] + acc[b, 9:12]), (name, b)
        assert cm[b].sum() == acc[b, 15] and np.trace(cm[b]) == acc[b, 16]
        # the whole matrix: the gather form restated in numpy, and the reference's resized pair
        assert np.array_equal(cm[b], E.resized_confusion(pred[b], target[b], dims[b])), (name, b)
        assert np.array_equal(cm[b], g[f"cm_{name}"][b]), (name, b)


def test_integer_index_rule_would_not_pass(golden):
    """The 512^2 sizes discriminate: a confusion matrix counted with d * in // out differs from
    the reference's in both images (so the test above cannot pass with that rule)."""
    g = golden("eval")
    logits, target, dims = case_tensors("c512")
    pred = logits.argmax(axis=1)
    for b, (oh, ow) in enumerate(dims):
        ry, rx = E.integer_rule_index(512, oh), E.integer_rule_index(512, ow)
        p, t = pred[b][ry][:, rx].ravel(), target[b][ry][:, rx].ravel()
        keep = t != 255
        cm = np.bincount(t[keep] * 3 + p[keep], minlength=9).reshape(3, 3)
        assert not np.array_equal(cm, g["cm_c512"][b])


@pytest.mark.parametrize("name", ["a64", "d37x50", "c512"])
def test_eval_confusion_without_dims_equals_argmax_dice_counts(ua, name):
    logits, target, _ = case_tensors(name)
    lg, tg = torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda()
    cm = ua.ops.eval_confusion(lg, tg).sum(dim=0)
    _, counts = ua.ops.argmax_dice_counts(lg, tg, want_preds=False)
    assert torch.equal(torch.diagonal(cm), counts[:, 0])
    assert torch.equal(cm.sum(dim=0), counts[:, 1])
    assert torch.equal(cm.sum(dim=1), counts[:, 2])
    # identity dims are the same thing
    H, W = logits.shape[2:]
    ident = torch.tensor([[H, W]] * logits.shape[0], dtype=torch.int64).cuda()
    assert torch.equal(ua.ops.eval_confusion(lg, tg, ident).sum(dim=0), cm)
    # an unaligned view of the same data takes the scalar path and counts the same
    pad = torch.empty(lg.numel() + 1, device="cuda")
    pad[1:] = lg.reshape(-1)
    assert torch.equal(ua.ops.eval_confusion(pad[1:].view_as(lg), tg).sum(dim=0), cm)


def test_out_of_range_dims_give_zero_counts_for_that_image_only(ua):
    logits, target, dims = case_tensors("a64")
    lg, tg = torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda()
    good = ua.ops.eval_confusion(lg, tg, torch.tensor(dims).cuda())
    for bad in ((0, 50), (64, 16385), (-3, 64), (1 << 40, 64)):
        d = torch.tensor(dims, dtype=torch.int64)
        d[1] = torch.tensor(bad)
        cm = ua.ops.eval_confusion(lg, tg, d.cuda())
        assert not cm[1].any(), bad
        assert torch.equal(cm[[0, 2, 3]], good[[0, 2, 3]]), bad
    # the extremes that are in range
    d = torch.tensor([(1, 1), (16384, 16384), (1, 16384), (64, 64)], dtype=torch.int64)
    cm = ua.ops.eval_confusion(lg, tg, d.cuda()).cpu().numpy()
    pred = logits.argmax(axis=1)
    assert cm[0].sum() == (target[0, 0, 0] != 255)
    for b in (0, 2):
        assert np.array_equal(cm[b], E.resized_confusion(pred[b], target[b], tuple(d[b].tolist())))
    # 64 -> 16384 is an exact 256x repeat
    assert np.array_equal(cm[1], 256 * 256 * E.resized_confusion(pred[1], target[1], (64, 64)))


@pytest.mark.parametrize("H,W,dims", [(16000, 4, [(500, 7), (16384, 3)]),
                                      (3, 15501, [(2, 9000), (5, 15501)])])
def test_network_sizes_too_large_for_the_lds_tables(ua, H, W, dims):
    """H + W beyond the LDS tables: every pixel's multiplicities are computed directly."""
    logits, target = E.make_case(77, len(dims), H, W)
    cm = ua.ops.eval_confusion(torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda(),
                               torch.tensor(dims, dtype=torch.int64).cuda()).cpu().numpy()
    pred = logits.argmax(axis=1)
    for b in range(len(dims)):
        assert np.array_equal(cm[b], E.resized_confusion(pred[b], target[b], dims[b])), b


def composed_confusion(logits, masks, dims):
    """Existing pieces on the same device logits: torch.argmax, per-image F.interpolate(nearest)
    of prediction and mask as the reference does it, torch.bincount."""
    preds = torch.argmax(logits, dim=1)
    total = torch.zeros(9, dtype=torch.int64, device=logits.device)
    for b, (oh, ow) in enumerate(dims):
        p = F.interpolate(preds[b][None, None].float(), size=(oh, ow), mode="nearest").long().view(-1)
        t = F.interpolate(masks[b][None, None].float(), size=(oh, ow), mode="nearest").long().view(-1)
        keep = t != 255
        total += torch.bincount(t[keep] * 3 + p[keep], minlength=9)
    return total.view(3, 3)


@pytest.mark.parametrize("size,dims", [
    (64, [(64, 64), (128, 128), (40, 50), (100, 150), (82, 94), (500, 375), (333, 500)]),
    (128, [(500, 375), (333, 500), (82, 94), (110, 164), (128, 128), (61, 300), (256, 256)]),
])
def test_evaluate_model_equals_the_composition_of_existing_pieces(ua, size, dims):
    """ua.UNet with seeded weights, a loader of batch size 3 over 7 images (so the last batch is
    partial): evaluate_model and evaluate_model_metrics equal, exactly, the metrics of the
    confusion matrix composed from model(images), torch.argmax, F.interpolate and bincount."""
    from oracle import unet_ref as O
    dev = torch.device("cuda", 0)
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(7))
    model = model.to(dev).eval()
    n = len(dims)
    images, _ = O.synthetic_batch(21 + size, n, size, size)
    masks = torch.from_numpy(E.make_case(300 + size, n, size, size)[1])
    loader = [{"image": images[i:i + 3], "mask": masks[i:i + 3],
               "original_dims": torch.tensor(dims[i:i + 3], dtype=torch.int64)}
              for i in range(0, n, 3)]
    assert [len(b["image"]) for b in loader] == [3, 3, 1]

    want = torch.zeros(3, 3, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for batch in loader:
            logits = model(batch["image"].to(dev))
            want += composed_confusion(logits, batch["mask"].to(dev), batch["original_dims"].tolist())
    ref = ua.SegmentationMetrics()
    ref.update_from_confusion(want.cpu())

    res = ua.evaluate.evaluate_model(model, loader, dev)
    assert np.array_equal(res["confusion_matrix"], want.cpu().numpy())
    assert res["pixel_accuracy"] == ref.compute_pixel_accuracy()
    assert res["mean_iou"] == ref.compute_mean_iou()
    for cls, name in enumerate(("background", "cat", "dog")):
        assert res[name] == {"dice": ref.compute_dice(cls), "iou": ref.compute_iou(cls),
                             "precision": ref.compute_precision(cls),
                             "recall": ref.compute_recall(cls)}
    assert res["mean_foreground_dice"] == (ref.compute_dice(1) + ref.compute_dice(2)) / 2
    assert set(res) == {"pixel_accuracy", "mean_iou", "background", "cat", "dog",
                        "mean_foreground_dice", "confusion_matrix"}
    assert ua.evaluate_model_metrics(model, loader, dev) == ref.get_all_metrics()
    # every prediction differs from a constant map, i.e. the counts are not trivial
    assert (want.sum(dim=0) > 0).sum() >= 2

    # predict_masks at the original sizes is the same nearest resize
    batch = loader[0]
    maps = ua.predict_masks(model, batch["image"].to(dev), batch["original_dims"])
    with torch.no_grad():
        preds = torch.argmax(model(batch["image"].to(dev)), dim=1)
    for b, (oh, ow) in enumerate(batch["original_dims"].tolist()):
        resized = F.interpolate(preds[b][None, None].float(), size=(oh, ow), mode="nearest")[0, 0]
        assert maps[b].dtype == torch.uint8 and torch.equal(maps[b], resized.to(torch.uint8))
    assert torch.equal(ua.predict_masks(model, batch["image"].to(dev)), preds.to(torch.uint8))


def test_metrics_accumulators_agree_between_the_old_and_the_new_path(ua):
    logits, target, _ = case_tensors("b128")
    lg, tg = torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda()
    old, new = ua.SegmentationMetrics(), ua.SegmentationMetrics()
    old.update_from_logits(lg, tg)
    new.update_from_logits(lg, tg, torch.tensor([[128, 128]] * 3))
    assert old.get_all_metrics() == new.get_all_metrics()
    for k in ("intersections", "unions", "true_positives", "false_positives", "false_negatives"):
        assert np.array_equal(getattr(old, k), getattr(new, k))
    assert old.total_pixels == new.total_pixels and old.correct_pixels == new.correct_pixels
    assert new.confusion_matrix.sum() == new.total_pixels
    with pytest.raises(RuntimeError, match="original_dims"):
        old.confusion_matrix
    pred = torch.argmax(lg, dim=1)
    assert ua.compute_dice(pred[0], tg[0], 1) == _single(ua, pred[0], tg[0]).compute_dice(1)
    assert ua.compute_iou(pred[0], tg[0], 0) == _single(ua, pred[0], tg[0]).compute_iou(0)
    assert ua.compute_pixel_accuracy(pred, tg) == old.compute_pixel_accuracy()


def _single(ua, pred, target):
    m = ua.SegmentationMetrics()
    m.update(pred, target)
    return m


@pytest.mark.parametrize("name", ["a64", "d37x50", "c512"])
def test_eval_maps_classes_errors_and_probabilities(ua, name):
    """Class map and error codes exact against a restatement; probabilities against float64
    softmax of the same logits, within twice the error torch's own fp32 softmax shows on these
    inputs on the same device (fp32 exp implementations differ by an ulp or two)."""
    logits, target, _ = case_tensors(name)
    lg, tg = torch.from_numpy(logits).cuda(), torch.from_numpy(target).cuda()
    probs, classes, errors = ua.ops.eval_maps(lg, tg)
    pred = torch.argmax(lg, dim=1)
    assert classes.dtype == torch.uint8 and torch.equal(classes.long(), pred)
    g = torch.where(tg == 255, torch.zeros_like(tg), tg)
    want = torch.zeros_like(tg)
    want[(pred > 0) & (g > 0) & (pred == g)] = 1
    want[(pred > 0) & (g == 0)] = 2
    want[(pred == 0) & (g > 0)] = 3
    want[(pred > 0) & (g > 0) & (pred != g)] = 4
    assert errors.dtype == torch.uint8 and torch.equal(errors.long(), want)
    assert len(torch.unique(want)) == 5
    exact = torch.softmax(lg.double(), dim=1)
    torch_err = (torch.softmax(lg, dim=1).double() - exact).abs().max().item()
    err = (probs.double() - exact).abs().max().item()
    print(f"softmax max abs error vs fp64 [{name}]: kernel {err:.3e}, torch fp32 {torch_err:.3e}")
    assert torch_err > 0 and err <= 2 * torch_err, (err, torch_err)
    # subsets of the outputs, and the unaligned (scalar) path
    p2, c2, e2 = ua.ops.eval_maps(lg, want_classes=False)
    assert c2 is None and e2 is None and torch.equal(p2, probs)
    pad = torch.empty(lg.numel() + 1, device="cuda")
    pad[1:] = lg.reshape(-1)
    p3, c3, e3 = ua.ops.eval_maps(pad[1:].view_as(lg), tg)
    assert torch.equal(p3, probs) and torch.equal(c3, classes) and torch.equal(e3, errors)


def test_confidence_and_error_maps_of_a_model(ua):
    from oracle import unet_ref as O
    dev = torch.device("cuda", 0)
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(7))
    model = model.to(dev).eval()
    images, _ = O.synthetic_batch(5, 2, 64, 64)
    masks = torch.from_numpy(E.make_case(9, 2, 64, 64)[1]).to(dev)
    with torch.no_grad():
        logits = model(images.to(dev))
    probs, _, errors = ua.ops.eval_maps(logits, masks)
    assert torch.equal(ua.evaluate.confidence_maps(model, images.to(dev)), probs)
    assert torch.equal(ua.evaluate.error_maps(model, images.to(dev), masks), errors)
    assert (probs.sum(dim=1) - 1).abs().max().item() <= 1e-6


def test_forward_and_eval_confusion_replay_from_a_hip_graph(ua):
    """The tail has no host dependency: forward + eval_confusion captured once, replayed on new
    inputs and new dims, give the counts of the eager call."""
    from oracle import unet_ref as O
    dev = torch.device("cuda", 0)
    model = ua.UNet()
    model.load_state_dict(O.fill_state_dict(7))
    model = model.to(dev).eval()
    img_a, _ = O.synthetic_batch(31, 2, 64, 64)
    img_b, _ = O.synthetic_batch(32, 2, 64, 64)
    tgt = [torch.from_numpy(E.make_case(s, 2, 64, 64)[1]).to(dev) for s in (41, 42)]
    dims = [torch.tensor(d, dtype=torch.int64, device=dev)
            for d in ([(82, 94), (100, 150)], [(500, 375), (40, 50)])]
    images, masks, d = img_a.to(dev).clone(), tgt[0].clone(), dims[0].clone()

    def tail():
        with torch.no_grad():
            return ua.ops.eval_confusion(model(images), masks, d)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tail()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tail()
    for im, tg, dd in ((img_a, tgt[0], dims[0]), (img_b, tgt[1], dims[1])):
        images.copy_(im.to(dev)); masks.copy_(tg); d.copy_(dd)
        graph.replay()
        got = out.clone()
        assert torch.equal(got, tail())
        assert got.sum().item() > 0
