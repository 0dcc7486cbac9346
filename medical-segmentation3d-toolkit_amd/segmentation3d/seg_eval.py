"""`seg_eval` command line -- the reference's segmentation3d/seg_eval.py without its hard-coded paths: score every case of
a test list against its ground truth with `cal_dsc_batch` and write the CSV.

    python -m segmentation3d.seg_eval -i test.txt --gt_folder GT --seg_folder SEG -l 1 2 -o results.csv [--surface]
                                   [--regions "1,2,3;1,3;3"] [--nsd_tolerance MM]
                                   [--lesionwise [--lesion_dilation N] [--lesion_min_voxels N] [--hd95_penalty X]]

Case names come from a list file (read_test_txt) or from the image files of a folder (read_test_folder); case <name> is
scored as <gt_folder>/<name>/<gt_name> against <seg_folder>/<name>/<seg_name>."""
import argparse
import os


def build_parser():
    parser = argparse.ArgumentParser(
        description='Dice (and optionally HD / HD95 / ASSD) of segmentations against ground-truth label volumes, '
                    'computed on an MI355X (HIP engine).')
    parser.add_argument('-i', '--input', required=True, help='test list file (.txt) or a folder of image files')
    parser.add_argument('--gt_folder', required=True, help='ground-truth root folder (one sub-folder per case)')
    parser.add_argument('--gt_name', default='seg.mha', help='file name of the ground-truth mask in a case folder')
    parser.add_argument('--seg_folder', required=True, help='segmentation root folder (one sub-folder per case)')
    parser.add_argument('--seg_name', default='seg.mha', help='file name of the segmentation in a case folder')
    parser.add_argument('-l', '--labels', type=int, nargs='+', required=True, help='labels to score')
    parser.add_argument('-t', '--threshold', type=int, default=10,
                        help='minimal voxel count for a label to count as present (TN / FP / FN / TP typing)')
    parser.add_argument('-o', '--output', default=None, help='result CSV file (default: print only)')
    parser.add_argument('--surface', action='store_true',
                        help='also report the Hausdorff distance, its 95th percentile and the average symmetric '
                             'surface distance (physical units) of every TP label')
    parser.add_argument('--regions', default=None,
                        help='overlapping regions to score as well, sets of label ids: "1,2,3;1,3;3" (BraTS whole tumour, '
                             'tumour core, enhancing tumour) adds region<k>_score / region<k>_type columns')
    parser.add_argument('--nsd_tolerance', type=float, default=None, metavar='MM',
                        help='with --surface: also report the normalized surface Dice at this tolerance in millimetres '
                             '(label<k>_nsd)')
    parser.add_argument('--lesionwise', action='store_true',
                        help='also report lesion-wise Dice / HD95, lesion counts and the lesion F1 of every label and '
                             'region (BraTS lesion-wise rule): <prefix>_lw_dice, _lw_hd95, _n_gt, _n_fn, _n_fp, _lesion_f1')
    parser.add_argument('--lesion_dilation', type=int, default=3, metavar='N',
                        help='18-neighbourhood dilations of the ground truth before it is split into lesions, 0..16')
    parser.add_argument('--lesion_min_voxels', type=int, default=1, metavar='N',
                        help='ground-truth lesions with fewer voxels are dropped (neither scored nor false negatives)')
    parser.add_argument('--hd95_penalty', type=float, default=374.0, metavar='X',
                        help='HD95 charged for every missed lesion and every spurious component')
    return parser


def lesion_options(args):
    """the lesion_options of cal_dsc_batch from the parsed command line"""
    return {'dilation_iters': args.lesion_dilation, 'min_lesion_voxels': args.lesion_min_voxels,
            'hd95_penalty': args.hd95_penalty}


def parse_regions(text):
    """'1,2,3;1,3;3' -> [[1, 2, 3], [1, 3], [3]]; None / '' -> None"""
    if not text:
        return None
    try:
        return [[int(l) for l in part.split(',')] for part in text.split(';')]
    except ValueError:
        raise ValueError('--regions must look like "1,2,3;1,3;3", got {!r}'.format(text))


def case_names(input_path):
    from segmentation3d.core.seg_infer import read_test_txt, read_test_folder
    if os.path.isdir(input_path):
        names, _ = read_test_folder(input_path)
    elif input_path.endswith('.txt'):
        names, _ = read_test_txt(input_path)
    else:
        raise ValueError('the input must be a .txt test list or a folder: {}'.format(input_path))
    return names


def main(argv=None):
    args = build_parser().parse_args(argv)
    from segmentation3d.core.seg_eval import cal_dsc_batch, check_lesion_kwargs
    from segmentation3d.utils.metrics import check_nsd_tolerance
    check_lesion_kwargs(lesion_options(args))          # bad values raise before the case list is read
    check_nsd_tolerance(args.nsd_tolerance)
    names = case_names(args.input)
    gt_files = [os.path.join(args.gt_folder, name, args.gt_name) for name in names]
    seg_files = [os.path.join(args.seg_folder, name, args.seg_name) for name in names]
    return cal_dsc_batch(gt_files, seg_files, args.labels, args.threshold, args.output,
                         surface_metrics=args.surface, regions=parse_regions(args.regions), lesionwise=args.lesionwise,
                         lesion_options=lesion_options(args), nsd_tolerance=args.nsd_tolerance)


if __name__ == '__main__':
    main()
