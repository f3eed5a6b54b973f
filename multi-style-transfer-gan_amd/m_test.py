"""Drop-in for the reference's m_test.py, its only evaluation of a trained model: ``calculate_fid`` (:37-50), ``process_image``
(:52-78) and the loop of ``run_model`` (:80-227) with the arithmetic on the GPU (mstg_hip.metrics.frechet_distance, csrc/frechet.hip;
mstg_hip.image.display_finish, csrc/display_finish.hip).

Differences from the reference, on purpose:
  * InceptionV3 is not part of this build (torchvision's weights come from the network): ``run_model`` takes the feature extractor
    from its caller, a callable from an (N, 3, H, W) cuda tensor in [-1, 1] to (N, D) features, and raises NotImplementedError
    without one.
  * ``calculate_fid`` works in float64 throughout (the reference's ``mean(0)`` of float32 features stays in float32) and takes
    ``tr sqrtm(S1 S2)`` as the nuclear norm of the n1 x n2 product of the centred features; more than
    ``mstg_hip.metrics.MAX_SAMPLES`` samples in BOTH sets are refused.
  * ``process_image`` clamps ``img * 0.5 + 0.5`` to [0, 1] before the power (the reference casts the NaN of a negative base).
  * The matplotlib figures are not built: each pair is written as one PNG, the two finished images side by side.
This file's name matches pytest's default pattern, so nothing here may be named like a test.
"""
from __future__ import annotations

import os

import numpy as np

from mstg_hip.metrics import calculate_fid  # noqa: F401  (part of this module's surface)

NO_EXTRACTOR = ("m_test.run_model: no feature_extractor given.  The reference builds torchvision's InceptionV3 with "
                "Inception_V3_Weights.DEFAULT, whose weights are downloaded; this build ships neither the network nor the weights.  "
                "Pass a callable from an (N, 3, H, W) cuda tensor to (N, D) features.")


def process_image(img_tensor):
    """(3, H, W) generator output in [-1, 1] on the GPU -> float64 (H, W, 3) numpy array in [0, 1]: the bytes of
    ``mstg_hip.image.display_finish`` over 255.0, as the reference's ``cv2.cvtColor(...) / 255.0``."""
    from mstg_hip import image as dimg
    return dimg.display_finish(img_tensor.detach())[0].cpu().numpy().astype(np.float64) / 255.0


def _features(extractor, x):
    f = extractor(x)
    return f.detach().cpu().numpy() if hasattr(f, "detach") else np.asarray(f)


def _translate(loader, generator, extractor, num_test, save_dir, stem):
    """one direction of the reference's loop (:124-165, :168-209): real and generated features of the first ``num_test`` items"""
    import torch
    from PIL import Image
    from mstg_hip import image as dimg
    real_features, fake_features = [], []
    for i, data in enumerate(loader):
        if i >= num_test:
            break
        real = data[0]
        with torch.no_grad():
            fake = generator(real)
        pair = dimg.display_finish(torch.cat([real[:1], fake[:1]]))  # both finishes in one batch
        Image.fromarray(np.concatenate(list(pair.cpu().numpy()), axis=1)).save(os.path.join(save_dir, "test_results", f"{stem}_{i}.png"))
        real_features.append(_features(extractor, real))
        fake_features.append(_features(extractor, fake))
    return np.concatenate(real_features), np.concatenate(fake_features)


def run_model(model_path, data_root, save_dir, num_test=100, feature_extractor=None):
    """The reference's test run: the first ``num_test`` test images of each domain through G_AB / G_BA (``G_AB_epoch_200.pth`` and
    ``G_BA_epoch_200.pth`` of ``model_path``), the finished pairs as PNG files, the two Frechet distances and their mean in
    ``test_results/test_results.txt``.  Returns (fid_monet2photo, fid_photo2monet)."""
    if feature_extractor is None:
        raise NotImplementedError(NO_EXTRACTOR)
    import torch
    from enhanced_train import EnhancedCycleGAN
    from pretrain import DeviceLoader, MonetPhotoDataset
    os.makedirs(os.path.join(save_dir, "test_results"), exist_ok=True)
    test_monet = MonetPhotoDataset(data_root, domain="A", split="test")
    test_photo = MonetPhotoDataset(data_root, domain="B", split="test")
    model = EnhancedCycleGAN()
    device = model.device
    model.G_AB.eval()
    model.G_BA.eval()
    model.G_AB.load_state_dict(torch.load(os.path.join(model_path, "G_AB_epoch_200.pth"), map_location=device, weights_only=True)["G_AB_state_dict"])
    model.G_BA.load_state_dict(torch.load(os.path.join(model_path, "G_BA_epoch_200.pth"), map_location=device, weights_only=True)["G_BA_state_dict"])
    real_monet, fake_photo = _translate(DeviceLoader(test_monet, batch_size=1, shuffle=False), model.G_AB, feature_extractor, num_test,
                                        save_dir, "monet2photo")
    real_photo, fake_monet = _translate(DeviceLoader(test_photo, batch_size=1, shuffle=False), model.G_BA, feature_extractor, num_test,
                                        save_dir, "photo2monet")
    fid_monet2photo = calculate_fid(real_photo, fake_photo)
    fid_photo2monet = calculate_fid(real_monet, fake_monet)
    with open(os.path.join(save_dir, "test_results", "test_results.txt"), "w") as f:
        f.write(f"test samples: {num_test}\n")
        f.write(f"Monet -> Photo FID: {fid_monet2photo:.4f}\n")
        f.write(f"Photo -> Monet FID: {fid_photo2monet:.4f}\n")
        f.write(f"mean FID: {(fid_monet2photo + fid_photo2monet) / 2:.4f}\n")
    return fid_monet2photo, fid_photo2monet
