"""Default training configuration -- same sections and keys as the reference's config/train_config.py:13-140
(general / dataset / loss / net / train / debug), so existing config files can be passed to `seg_train -i` unchanged."""
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import FixedNormalizer, AdaptiveNormalizer  # noqa: F401

__C = edict()
cfg = __C

__C.general = {}
__C.general.imseg_list = '/path/to/train.csv'          # image / segmentation pair list
__C.general.save_dir = '/tmp/seg3d_model'              # models, logs and checkpoints go here
__C.general.model_scale = 'fine'                       # sub-folder of save_dir ('coarse' / 'fine' / ...)
__C.general.resume_epoch = -1                          # >= 0: continue from that checkpoint
__C.general.num_gpus = 1                               # > 0 (one process per GPU; the HIP engine has no CPU path)
__C.general.seed = 0

__C.dataset = {}
__C.dataset.num_classes = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]                  # mm, (x, y, z)
__C.dataset.crop_size = [96, 96, 96]                   # voxels, multiples of max_stride (16)
__C.dataset.sampling_method = 'HYBRID'                 # GLOBAL | MASK | HYBRID | CENTER
__C.dataset.random_translation = [15, 15, 15]             # mm, uniform in [-t, t] per axis
__C.dataset.random_scale = [0.9, 1.1]                     # crop spacing = spacing * uniform(lo, hi)
__C.dataset.random_mirror_axes = []                       # e.g. ['x', 'y']: mirror each listed axis with probability 1/2
__C.dataset.interpolation = 'LINEAR'                   # NN | LINEAR | BSPLINE
# on-device training augmentation (an extension of this build, everything off: the crops and the RNG stream are then
# exactly those without the section).  Rotation and elastic deformation run inside the crop's resampling launch, the
# intensity transforms in one fused pass over the normalised crop.  A transform is on when its probability is > 0 and
# its range is not neutral; an nnU-Net-like setting is noted behind each key.
__C.dataset.augmentation = {}
__C.dataset.augmentation.rotation_deg = [0, 0, 0]         # per-axis max angle (x, y, z), uniform in [-a, a]   ([30, 30, 30])
__C.dataset.augmentation.rotation_prob = 1.0              #                                                     (0.2)
__C.dataset.augmentation.elastic_grid_mm = 32.0           # control-point spacing of the cubic B-spline field
__C.dataset.augmentation.elastic_magnitude_mm = [0, 0]    # control displacements uniform in [-a, a], a in [lo, hi]; hi < grid / 6   ([0, 4])
__C.dataset.augmentation.elastic_prob = 0.0               #                                                     (0.2)
__C.dataset.augmentation.brightness = [1, 1]              # multiplicative, uniform in [lo, hi]                 ([0.75, 1.25])
__C.dataset.augmentation.brightness_prob = 0.0            #                                                     (0.15)
__C.dataset.augmentation.contrast = [1, 1]                # about the crop's mean, range preserved              ([0.75, 1.25])
__C.dataset.augmentation.contrast_prob = 0.0              #                                                     (0.15)
__C.dataset.augmentation.gamma = [1, 1]                   # on the crop's range                                 ([0.7, 1.5])
__C.dataset.augmentation.gamma_prob = 0.0                 #                                                     (0.3)
__C.dataset.augmentation.gamma_invert_prob = 0.0          # gamma on the inverted range                         (0.25)
__C.dataset.augmentation.noise_sigma = [0, 0]             # additive Gaussian noise on the normalised crop      ([0, 0.1])
__C.dataset.augmentation.noise_prob = 0.0                 #                                                     (0.1)
__C.dataset.crop_normalizers = [AdaptiveNormalizer()]

__C.loss = {}
__C.loss.name = 'Dice'                                 # Focal | Dice | CE
__C.loss.obj_weight = [1 / 2, 1 / 2]                   # per-class weights (normalised to sum 1)
__C.loss.focal_gamma = 2

__C.net = {}
__C.net.name = 'vbnet'                                 # plugin module under segmentation3d.network

__C.train = {}
__C.train.epochs = 1001
__C.train.batchsize = 4                                # per GPU
__C.train.num_threads = 4
__C.train.lr = 1e-4
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 100
# extensions of this build (absent keys mean the reference's behaviour: fp32, eager steps)
__C.train.compute_dtype = 'fp32'                       # 'bf16': bf16 activations / packed weights, fp32 accumulate + master weights
__C.train.use_graph = False                            # capture the whole train step in one hipGraph (single process only)
__C.train.gc_freeze = True                             # gc.freeze() after the first steps: short collector pauses in the eager loop

__C.debug = {}
__C.debug.save_inputs = False
