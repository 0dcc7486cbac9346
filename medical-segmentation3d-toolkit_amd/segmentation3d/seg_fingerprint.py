"""`seg_fingerprint` command line -- the intensity fingerprint of a training list: per modality the foreground (mask > 0)
percentiles, mean and standard deviation over ALL cases, i.e. the numbers of a ClipZScoreNormalizer for CT-like data.

    python -m segmentation3d.seg_fingerprint -i train.txt [--percentiles 0.5 99.5] [--gpu 0]

Prints one ready-to-paste `ClipZScoreNormalizer(mean, stddev, lower, upper)` line per modality, plus n, min and max.  The
percentiles are nearest-rank order statistics of the pooled foreground voxels, exact; the statistics are computed on the
device (dataloader.dataset.intensity_fingerprint)."""
import argparse


def build_parser():
    parser = argparse.ArgumentParser(
        description='Foreground intensity statistics of a training list, computed on an MI355X (HIP engine).')
    parser.add_argument('-i', '--input', required=True, help='training list file (.txt or .csv)')
    parser.add_argument('--percentiles', type=float, nargs=2, default=[0.5, 99.5], metavar=('LO', 'HI'),
                        help='clip percentiles in percent')
    parser.add_argument('--gpu', type=int, default=0, help='device ordinal')
    return parser


def format_lines(stats):
    """the report of intensity_fingerprint's result, one block of two lines per modality"""
    lines = []
    for m, st in enumerate(stats):
        lines.append('# modality {}: n = {}, min = {!r}, max = {!r}'.format(m, st['n'], st['min'], st['max']))
        lines.append('ClipZScoreNormalizer({!r}, {!r}, {!r}, {!r})'.format(st['mean'], st['std'], st['lower'], st['upper']))
    return lines


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from segmentation3d.dataloader.dataset import intensity_fingerprint
    stats = intensity_fingerprint(args.input, tuple(args.percentiles), torch.device('cuda', args.gpu))
    for line in format_lines(stats):
        print(line)
    return stats


if __name__ == '__main__':
    main()
