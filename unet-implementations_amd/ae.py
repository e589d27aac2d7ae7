"""The autoencoder pretraining loop of AE_pretrained/reconstruction/src/train.py on the HIP path
(`ua.ae`): phase 1 of the reference's transfer-learning recipe, whose checkpoint's encoder
`UNet.load_pretrained_encoder` loads for phase 2.

Function for function: `create_model` (:340-375), `create_optimizer` (:377-397),
`create_lr_scheduler` (:399-418), `get_loss_function` (:420-437), `validate` (:440-498),
`train_one_epoch` (:501-554), `save_checkpoint` (:556-600) and `load_checkpoint`; and
`evaluate_reconstruction_quality` of src/evaluate.py:268-377.  The step order
is the reference's, so `ua.train_step` / `ua.GraphedTrainStep` run it unchanged.
"""
import math
import os

import torch

from . import ops
from .autoencoder import Autoencoder
from .losses import MSELoss, PerceptualLoss, ReconstructionLoss
from .optim import FusedAdam
from .train import train_step


def create_model(device="cuda"):
    """The exact configuration built at src/train.py:340-375 (lower dropout than the UNet's)."""
    model = Autoencoder(in_channels=3, out_channels=3, n_stages=6,
                        features_per_stage=[32, 64, 128, 256, 512, 512],
                        kernel_sizes=[[3, 3]] * 6,
                        strides=[[1, 1], [2, 2], [2, 2], [2, 2], [2, 2], [2, 2]],
                        n_conv_per_stage=[2] * 6, n_conv_per_stage_decoder=[2] * 5,
                        conv_bias=True, norm_op=torch.nn.InstanceNorm2d,
                        norm_op_kwargs={"eps": 1e-5, "affine": True}, dropout_op=None,
                        nonlin=torch.nn.LeakyReLU, nonlin_kwargs={"inplace": True},
                        encoder_dropout_rates=[0.0, 0.0, 0.05, 0.1, 0.15, 0.15],
                        decoder_dropout_rates=[0.15, 0.1, 0.1, 0.05, 0.0])
    return model.to(device)


def create_optimizer(model, lr=1e-3, weight_decay=1e-5):
    """Adam as at src/train.py:377-397 (defaults from the reference's argument parser)."""
    return FusedAdam(model.parameters(), lr=lr, weight_decay=weight_decay, model=model)


def create_lr_scheduler(optimizer, max_epochs):
    """Cosine annealing to 1e-6 over the run, stepped per epoch (src/train.py:399-418)."""
    return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=max_epochs, eta_min=1e-6)


def get_loss_function(device=None, target_layout="nchw"):
    """nn.MSELoss() (src/train.py:420-437)."""
    return MSELoss(target_layout=target_layout)


def get_reconstruction_loss(mse_weight=1.0, perceptual_weight=0.0, ssim_weight=0.0,
                            perceptual_layers=None, target_layout="nchw", device=None):
    """The loss the reference ships and documents - ReconstructionLoss(mse_weight,
    perceptual_weight, ssim_weight) of models/losses.py:12-79, the recorded run's
    training_config.json holding 1.0 / 0.1 / 0.1 - which its own get_loss_function never builds
    (src/train.py:420-437 returns nn.MSELoss() although --perceptual_weight is parsed and written
    to the config).  With perceptual_weight > 0 the random VGG16 trunk is drawn here, from torch's
    global generator, as the reference's constructor does.  `device`: where to put the loss (its
    trunk's weights and buffers); None leaves it on the CPU for the caller's `.to(device)`."""
    perceptual = None
    if perceptual_weight > 0:
        perceptual = PerceptualLoss(layers=perceptual_layers, target_layout=target_layout)
    loss = ReconstructionLoss(mse_weight, perceptual_weight, ssim_weight,
                              target_layout=target_layout, perceptual=perceptual)
    return loss if device is None else loss.to(device)


def train_one_epoch(model, train_loader, optimizer, loss_function, device, scaler=None):
    """src/train.py:501-554 without the per-step `loss.item()` sync: the losses are summed on the
    device and read once at the end."""
    if scaler is not None:
        raise NotImplementedError("fp16 GradScaler AMP is not part of the HIP path "
                                  "(use matmul_precision='bf16')")
    model.train()
    total = torch.zeros((), device=device)
    n = 0
    for batch in train_loader:
        images = batch["image"].to(device, non_blocking=True)
        targets = batch["target"].to(device, non_blocking=True)
        total += train_step(model, optimizer, loss_function, images, targets)
        n += 1
    return (total / max(n, 1)).item()


@torch.no_grad()
def validate(model, val_loader, loss_function, device):
    """src/train.py:440-498: eval-mode loss averaged over batches; per-image MSE and
    PSNR = 10 log10(1 / mse) summed over images and divided by the dataset size.  Everything stays
    on the device (the per-image sums come out of the loss kernel); one sync at the end.
    Returns (val_loss, {"loss", "mse", "psnr"})."""
    model.eval()
    val_loss = torch.zeros((), device=device, dtype=torch.float64)
    mse_sum = torch.zeros((), device=device, dtype=torch.float64)
    psnr_sum = torch.zeros((), device=device, dtype=torch.float64)
    batches = 0
    for batch in val_loader:
        images = batch["image"].to(device, non_blocking=True)
        targets = batch["target"].to(device, non_blocking=True)
        outputs = model(images)
        val_loss += loss_function(outputs, targets).double()
        N, C, H, W = outputs.shape
        mse = (loss_function.last_per_image / (C * H * W)).float()    # per image, fp32
        mse_sum += mse.double().sum()
        psnr_sum += (10 * torch.log10(1.0 / mse)).double().sum()
        batches += 1
    ds = getattr(val_loader, "dataset", None)
    num_samples = len(ds) if ds is not None else None
    vals = torch.stack([val_loss, mse_sum, psnr_sum]).tolist()
    if num_samples is None:
        raise TypeError("validate needs a DataLoader-like object with a .dataset")
    loss = vals[0] / max(batches, 1)
    metrics = {"loss": loss, "mse": vals[1] / num_samples, "psnr": vals[2] / num_samples}
    return loss, metrics


@torch.no_grad()
def evaluate_reconstruction_quality(model, test_loader, device, output_dir=None,
                                    visualize_samples=0):
    """src/evaluate.py:268-377: eval mode, per-image MSE, PSNR and SSIM (calculate_psnr /
    calculate_ssim) summed over the test set and divided by the number of images.  One fused
    forward per batch gives all three; the sums stay on the device and are read once at the end.
    Returns {"mse", "psnr", "ssim", "num_samples"}.

    With `visualize_samples > 0` and an `output_dir`, the first `visualize_samples` images each
    leave `visualizations/comparison_{i}_{name}` there (src/evaluate.py:333-368): original |
    reconstruction | error map, rendered on the device (`ops.render_recon_panels`, DESIGN.md
    section 9b) and written as PNG.  `name` is the batch's `filename` entry, or `sample_{i}.png`;
    `.png` is appended to a name with another extension.  The metrics are those of a
    `visualize_samples=0` run.  Without an `output_dir`, `visualize_samples > 0` raises."""
    if visualize_samples > 0 and output_dir is None:
        raise NotImplementedError("reconstruction visualisations are not part of the HIP path "
                                  "(use visualize_samples=0)")
    vis_dir, written = None, 0
    if visualize_samples > 0:
        from .render import write_png
        vis_dir = os.path.join(str(output_dir), "visualizations")
        os.makedirs(vis_dir, exist_ok=True)
    model.eval()
    sums = torch.zeros(3, device=device, dtype=torch.float64)
    num_samples = 0
    for batch in test_loader:
        images = batch["image"].to(device, non_blocking=True)
        targets = batch["target"].to(device, non_blocking=True)
        recon = model(images).contiguous().float()
        if written < visualize_samples:
            k = min(images.shape[0], visualize_samples - written)
            names = batch.get("filename") if hasattr(batch, "get") else None
            panels = ops.render_recon_panels(images[:k], recon[:k])
            for j in range(k):
                name = str(names[j]) if names is not None else f"sample_{written}.png"
                if not name.lower().endswith(".png"):
                    name += ".png"
                H, P, W, _ = panels[j].shape
                write_png(os.path.join(vis_dir, f"comparison_{written}_{name}"),
                          panels[j].view(H, P * W, 3))
                written += 1
        u8 = targets.dtype == torch.uint8
        if not u8 and targets.dtype != torch.float32:
            targets = targets.float()
        _, ssim, sq = ops.ssim_fwd(recon, targets.contiguous(), u8, want_loss=False)
        N, C, H, W = recon.shape
        mse = (sq / (C * H * W)).float()
        psnr = 10 * torch.log10(1.0 / torch.clamp(mse, min=1e-10))
        sums += torch.stack([mse.double().sum(), psnr.double().sum(), ssim.float().double().sum()])
        num_samples += N
    if num_samples == 0:
        raise ValueError("evaluate_reconstruction_quality: empty test loader")
    mse, psnr, ssim = (v / num_samples for v in sums.tolist())
    return {"mse": mse, "psnr": psnr, "ssim": ssim, "num_samples": num_samples}


@torch.no_grad()
def analyze_latent_space(model, test_loader, device, output_dir, perplexity=30.0):
    """src/evaluate.py:380-440: eval mode, `model.encode` of every test image, the codes reduced to
    2-D with PCA and with t-SNE, and the two scatter pictures coloured by `batch["label"]` written
    to `latent_analysis/latent_space_pca.png` and `latent_space_tsne.png` under `output_dir`.
    The codes go straight into one preallocated device matrix [len(dataset), D]; one centred Gram
    matrix (`latent.gram`) serves both reductions, the t-SNE starting from the PCA scores.
    Returns {"pca", "tsne" (the [N, 2] coordinates), "labels", "kl_divergence", "n_iter",
    "pca_residuals", "explained_variance", "num_samples"}; the reference returns nothing."""
    from . import latent
    from .render import write_png
    ds = getattr(test_loader, "dataset", None)
    if ds is None:
        raise TypeError("analyze_latent_space needs a DataLoader-like object with a .dataset")
    total = len(ds)
    latent_dir = os.path.join(str(output_dir), "latent_analysis")
    os.makedirs(latent_dir, exist_ok=True)
    model.eval()
    codes, labels, n = None, torch.empty(total, dtype=torch.int64, device=device), 0
    for batch in test_loader:
        if "label" not in batch:
            raise KeyError("label: analyze_latent_space colours the codes by batch['label'] (the "
                           "reference's dataset yields int(mask.max()) per image)")
        images = batch["image"].to(device, non_blocking=True)
        z = model.encode(images)
        if codes is None:
            codes = torch.empty((total, z.shape[1]), dtype=torch.float32, device=device)
        B = z.shape[0]
        if n + B > total:
            raise ValueError("analyze_latent_space: the loader yields more images than its dataset")
        codes[n:n + B] = z
        labels[n:n + B] = torch.as_tensor(batch["label"]).to(device).reshape(-1)
        n += B
    if n < 2:
        raise ValueError("analyze_latent_space: fewer than two test images")
    codes, labels = codes[:n], labels[:n]
    G = latent.gram(codes)
    pca = latent.pca_2d(G)
    write_png(os.path.join(latent_dir, "latent_space_pca.png"),
              latent.scatter_figure(pca.scores, labels))
    s = pca.scores.double()
    tsne = latent.tsne_2d(G, perplexity=perplexity, init=s / s[:, 0].std(unbiased=False) * 1e-4)
    write_png(os.path.join(latent_dir, "latent_space_tsne.png"),
              latent.scatter_figure(tsne.y, labels))
    return {"pca": pca.scores, "tsne": tsne.y, "labels": labels,
            "kl_divergence": tsne.kl_divergence, "n_iter": tsne.n_iter,
            "pca_residuals": pca.residuals, "explained_variance": pca.explained_variance,
            "num_samples": n}


def save_checkpoint(model, optimizer, scheduler, epoch, best_loss, output_dir, is_best=False):
    """Same files and dictionary keys as src/train.py:556-600 (`best_loss`,
    `config.out_channels`); the config records the model's actual geometry."""
    ckpt_dir = os.path.join(str(output_dir), "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    n = model.n_stages
    checkpoint = {
        "epoch": epoch,
        "model_state_dict": model.state_dict(),
        "optimizer_state_dict": optimizer.state_dict(),
        "scheduler_state_dict": scheduler.state_dict() if scheduler is not None else None,
        "best_loss": best_loss,
        "config": {"in_channels": model.in_channels, "out_channels": model.out_channels,
                   "n_stages": n, "features_per_stage": list(model.features_per_stage),
                   "kernel_sizes": [[3, 3]] * n, "strides": [[1, 1]] + [[2, 2]] * (n - 1),
                   "n_conv_per_stage": [2] * n, "n_conv_per_stage_decoder": [2] * (n - 1),
                   "conv_bias": True, "norm_op_kwargs": {"eps": 1e-5, "affine": True},
                   "nonlin_kwargs": {"inplace": True}},
    }
    path = os.path.join(ckpt_dir, f"checkpoint_epoch_{epoch}.pth")
    torch.save(checkpoint, path)
    if is_best:
        torch.save(checkpoint, os.path.join(str(output_dir), "best_model.pth"))
    return path


def load_checkpoint(path, model, optimizer=None, scheduler=None, device="cuda"):
    """Resume from a save_checkpoint file; returns (start_epoch, best_loss)."""
    checkpoint = torch.load(path, map_location=device, weights_only=True)
    model.load_state_dict(checkpoint["model_state_dict"])
    if optimizer is not None and checkpoint.get("optimizer_state_dict") is not None:
        optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
    if scheduler is not None and checkpoint.get("scheduler_state_dict") is not None:
        scheduler.load_state_dict(checkpoint["scheduler_state_dict"])
    return checkpoint["epoch"] + 1, checkpoint.get("best_loss", math.inf)
