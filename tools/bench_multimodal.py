"""Multi-modality data path on one GPU (prints one JSON line; --out FILE also writes it):
  (i)   GB/s of seg3d_patch_gather_normalize_mc (16 patches of 96^3 x 4 modalities, adaptive normalisers) and of the
        training crop (seg3d_resample_affine_mc + the in-place mc normalisation, 96^3 x 4), on algorithmic bytes, against
        the 8 TB/s HBM peak;
  (ii)  whole-volume inference seconds of a synthetic 4-modality 240 x 240 x 155 volume (96^3 boxes, stride 48, vnet(4, 2),
        hipGraph replay) and the share of that time the gathers take (gather time per batch, measured alone, x batches);
  (iii) the train-step time of vnet(4, 4) at 4 x 96^3 fed by the file-backed dataset (two .mha cases per modality, crops
        and batches on the device) next to the same step on a resident synthetic batch.
usage: python tools/bench_multimodal.py [--steps K] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'medical-segmentation3d-toolkit_amd'))
sys.path.insert(0, REPO)

HBM_PEAK = 8.0e12
M = 4


def _events_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def gather_and_crop(dev, vol, reps=50):
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    from segmentation3d.utils import image_tools
    Z, Y, X, _ = vol.shape
    box, P = (96, 96, 96), 16
    rng = np.random.RandomState(0)
    starts = [[int(rng.randint(0, X - 96 + 1)), int(rng.randint(0, Y - 96 + 1)), int(rng.randint(0, Z - 96 + 1))]
              for _ in range(P)]
    norms = [{'type': 1, 'clip_sigma': 3}] * M
    batcher = SlidingWindowBatcher(vol, starts, box, 2, norms, max_batch=P)
    batcher.set_batch(list(range(P)))
    out = batcher.gather_current()
    ms = _events_ms(lambda: batcher.gather_current(out=out), reps)
    patch_bytes = P * 96 ** 3 * M * 4
    gather_bytes = 3 * patch_bytes            # stats pass reads, gather reads, gather writes
    # training crop: one source row per output voxel read + the crop written, then the in-place normalisation
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    params = image_tools.normalizer_params(norms, M)
    crop = torch.empty((96, 96, 96, M), dtype=torch.float32, device=dev)
    center = (X / 2.0, Y / 2.0, Z / 2.0)

    def one_crop():
        image_tools.crop_image_device_mc(vol, frame, center, (96, 96, 96), (1.1, 1.1, 1.1), 'LINEAR', out=crop)
        image_tools.normalize_crop_device_mc(crop, params, out=crop)
    crop_ms = _events_ms(one_crop, reps)
    crop_bytes = 2 * 96 ** 3 * M * 4 + 3 * 96 ** 3 * M * 4
    return {'gather_16x96^3x4_ms': ms, 'gather_GBps': gather_bytes / (ms * 1e-3) / 1e9,
            'gather_frac_of_hbm_peak': gather_bytes / (ms * 1e-3) / HBM_PEAK, 'gather_bytes': gather_bytes,
            'crop_96^3x4_ms': crop_ms, 'crop_GBps': crop_bytes / (crop_ms * 1e-3) / 1e9,
            'crop_frac_of_hbm_peak': crop_bytes / (crop_ms * 1e-3) / HBM_PEAK}, ms


def whole_volume(dev, gather_ms):
    from segmentation3d.core.seg_infer import sliding_window_inference
    from segmentation3d.network import vnet
    from segmentation3d.utils.image_tools import image_partition_by_fixed_size
    torch.manual_seed(0)
    net = vnet.SegmentationNet(M, 2)
    vnet.parameters_kaiming_init(net)
    net = net.to(dev).eval()
    X, Y, Z = 240, 240, 160                     # 155 planes padded to the stride multiple, as segmentation_volume does
    vol = torch.randn((Z, Y, X, M), device=dev) * 100
    starts, _ = image_partition_by_fixed_size(((X, Y, Z), (1.0, 1.0, 1.0)), [0, 0, 0], [X, Y, Z], [96.0] * 3, [48.0] * 3, 16)
    norms = [{'type': 1, 'clip_sigma': 3}] * M
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sliding_window_inference(net, vol, starts, (96, 96, 96), 2, norms, batch_size=16)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    batches = (len(starts) + 15) // 16
    best = min(times[1:])
    return {'volume_xyzm': [X, Y, Z, M], 'patches': len(starts), 'infer_s': best, 'infer_s_runs': times,
            'gather_share': batches * gather_ms * 1e-3 / best}


def train_steps(dev, steps):
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.dataloader.dataset import SegmentationDataset, DeviceCropLoader
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    tmp = tempfile.mkdtemp(prefix='mm_bench_')
    rng = np.random.RandomState(1)
    lines = []
    for k in range(2):
        seg = (rng.rand(128, 144, 160) > 0.7).astype(np.int8) * (1 + k)
        for m in range(M):
            p = os.path.join(tmp, 'c{}_m{}.mha'.format(k, m))
            write_mha(Image3d((rng.randn(128, 144, 160) * 50 + 10 * m).astype(np.float32)), p)
            lines.append(p)
        p = os.path.join(tmp, 'c{}_seg.mha'.format(k))
        write_mha(Image3d(seg), p)
        lines.append(p)
    lst = os.path.join(tmp, 'train.txt')
    with open(lst, 'w') as f:
        f.write('2 {}\n'.format(M) + '\n'.join(lines) + '\n')
    ds = SegmentationDataset(lst, 4, [1.0, 1.0, 1.0], [96, 96, 96], 'GLOBAL', [5, 5, 5], [0.9, 1.1], 'LINEAR',
                             [AdaptiveNormalizer()] * M, device=dev)
    step = TrainStep('vnet', M, 4, 'Dice', [0.25] * 4, device=dev, seed=0)
    np.random.seed(0)
    n = steps + 3
    loader = iter(DeviceCropLoader(ds, [k % 2 for k in range(4 * n)], 4))
    for _ in range(3):
        crops, masks, _, _ = next(loader)
        step(crops, masks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        crops, masks, _, _ = next(loader)
        step(crops, masks)
    torch.cuda.synchronize()
    file_ms = (time.perf_counter() - t0) / steps * 1e3
    x = torch.randn((4, 96, 96, 96, M), device=dev).permute(0, 4, 1, 2, 3)
    t = torch.randint(0, 4, (4, 1, 96, 96, 96), device=dev).float()
    for _ in range(3):
        step(x, t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step(x, t)
    torch.cuda.synchronize()
    resident_ms = (time.perf_counter() - t0) / steps * 1e3
    return {'train_step_file_backed_ms': file_ms, 'train_step_resident_ms': resident_ms,
            'data_path_overhead_ms': file_ms - resident_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from segmentation3d import _engine
    _engine.lib()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    vol = (torch.randn((155, 240, 240, M), device=dev) * 100).contiguous()
    r = {'device': torch.cuda.get_device_name(0)}
    g, gather_ms = gather_and_crop(dev, vol)
    r.update(g)
    del vol
    r.update(whole_volume(dev, gather_ms))
    r.update(train_steps(dev, a.steps))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
