"""Command-line flags of the hot-path scripts.  Names and defaults are the reference's
(src/arguments.py:3-68, plus behavioral_cloning/save_embedded_obs.py:25-26); the only additions are the
MI355X knobs at the end.  A fresh parser is built per call (the reference mutates one module-level parser,
which makes a second import of a script fail with an argparse conflict, cf. main_test.py:14)."""
import argparse


def make_parser():
    parser = argparse.ArgumentParser(description='PyTorch Scalable Agent')
    # Behavioral Cloning Settings.
    parser.add_argument('--max_frames', type=int, default=200000000)
    parser.add_argument('--n_episodes_test', type=int, default=50)
    parser.add_argument('--eval_frequency', type=int, default=200)
    parser.add_argument('--to_env', type=str, default='HabitatImageNav-apartment_0')
    parser.add_argument('--debug', action='store_true')
    parser.add_argument('--disable_save', action='store_true')
    parser.add_argument('--essential_save_only', action='store_true')
    parser.add_argument('--save_path', type=str, default='bc')
    parser.add_argument('--data_path', type=str, default='behavioral_cloning')
    # Embedding Settings.
    parser.add_argument('--embedding_name', type=str, default='resnet50')
    parser.add_argument('--train_embedding', action='store_true',
                        help='EmbeddingNet(train=True): a trainable fp32 encoder on one GPU - resnet18 / resnet34 / resnet50 and the conv5 checkpoints; '
                             'every other name, and save_embedded_obs (embedding rows need the frozen encoder), refuse it.  main_bc_finetune: '
                             'end-to-end BC - the encoder named by --embedding_name in front of PolicyNet on the raw frames, one clip and RMSprop '
                             'update over both (fused, or the reference lines with --autograd_step); the training workspace grows with '
                             'unroll_length x batch_size x frames and is checked against the free device memory before the first step')
    parser.add_argument('--disable_pretrained_embedding', action='store_false', dest='pretrained_embedding')
    # not in the reference: fine-tuning with frozen BatchNorm, which lifts the frame limit of --train_embedding
    parser.add_argument('--freeze_embedding_bn', action='store_true',
                        help='with --train_embedding: frozen BatchNorm (torch: model.train() then .eval() on every BatchNorm) - the convolutions and the '
                             'BatchNorm affine parameters train, BatchNorm normalises with the running statistics of the checkpoint and leaves them '
                             'unchanged.  Frames are then independent, a step runs as passes of --embedding_chunk frames and the training workspace is '
                             'sized by the chunk: any unroll_length x batch_size trains')
    parser.add_argument('--embedding_chunk', type=int, default=None,
                        help='with --freeze_embedding_bn: frames per trainer pass (default: the largest count within the trainer\'s own limit - 668 frames '
                             'for resnet18 / 34, 334 for resnet50 - whose workspace fits the free device memory, never above unroll_length x batch_size x '
                             'frames)')
    parser.add_argument('--embedding_wgrad_split16', action='store_true',
                        help='with --train_embedding: every weight gradient of the encoder, conv1\'s included, as an exact-split product on the f16 matrix '
                             'pipe (per-tensor power-of-two scales, three MFMAs per fragment pair, fp32 accumulation: about 2^-22 relative to the fp32 '
                             'path); the forward, the data gradients and BatchNorm stay fp32.  Works with and without --freeze_embedding_bn')
    parser.add_argument('--embedding_conv_split16', action='store_true',
                        help='with --train_embedding: every forward convolution and data gradient of the encoder\'s layer1 .. layer4 as an exact-split '
                             'product on the f16 matrix pipe (both operands scaled per tensor on the device, three MFMAs per fragment pair, fp32 '
                             'accumulation: about 2^-22 relative per product); conv1, BatchNorm and the pools stay fp32, the weight gradients too unless '
                             '--embedding_wgrad_split16 is given as well.  Works with and without --freeze_embedding_bn')
    parser.add_argument('--embedding_train_from', type=str, default=None, choices=['layer1', 'layer2', 'layer3', 'layer4'],
                        help='with --train_embedding: partial fine-tuning - the named stage of the ResNet trunk and the ones above it train; conv1 / bn1 '
                             'and the stages below are frozen (eval-mode BatchNorm, no gradient), keep no activations and have no backward, so the '
                             'training workspace and the step shrink with the stage and the default --embedding_chunk grows.  Works with and without '
                             '--freeze_embedding_bn and the split16 modes; a resumed run must name the same stage')
    parser.add_argument('--embedding_prefix_once', action='store_true',
                        help='with --embedding_train_from: the frozen prefix runs once per frame and step - its one output, the boundary tensor, is kept '
                             'for the unroll_length x batch_size x frames frames of a step (0.2 .. 3.2 MB per frame, counted next to the workspace) and '
                             'the recompute passes of a --freeze_embedding_bn step start at the first trained stage; with --embedding_conv_split16 a '
                             'prefix convolution and its BatchNorm are one launch.  The bits do not change: a run may be resumed with or without it')
    parser.add_argument('--embedding_prefix_cache', action='store_true',
                        help='with --embedding_train_from: the frozen prefix runs once per DATASET frame - before training the boundary tensor of every '
                             'frame of the scene is computed into one device tensor (samples x frames x 0.2 .. 3.2 MB, counted with a pass\'s staging '
                             'tensor next to the workspace; a cache that does not fit is refused with both sizes), and every pass of a step gathers '
                             'its frames\' rows and starts at the first trained stage.  Replaces the step-sized cache of --embedding_prefix_once.  The '
                             'bits do not change: a run may be resumed with or without it (the cache is rebuilt)')
    parser.add_argument('--embedding_random_crop', action='store_true',
                        help='with --train_embedding: every frame of a training step goes through Resize(256) and then its own random 224 x 224 window '
                             'of the resized frame instead of the centre one (one launch writes the windowed image; evaluation keeps the centre crop).  '
                             'The windows are a function of --run_id, the iteration and the frame, so a resumed run draws what an uninterrupted one '
                             'would, and a run may be resumed with or without the flag.  Not with --embedding_prefix_cache, whose cache holds the '
                             'frozen prefix\'s output for ONE window per frame; --embedding_prefix_once is the compatible mode')
    parser.add_argument('--embedding_color_jitter', type=float, nargs=3, default=None, metavar=('B', 'C', 'S'),
                        help='with --train_embedding: every frame of a training step gets its own brightness, contrast and saturation factor, each '
                             'uniform in [max(0, 1 - strength), 1 + strength] for the strengths B, C and S, applied in a random order per frame to the '
                             'uint8 values of its 224 x 224 window, as torchvision\'s ColorJitter does (hue is not offered; evaluation keeps the un-jittered '
                             'centre crop).  Default off; 0 0 0 is off too.  The factors are a function of --run_id, the iteration and the frame, so a '
                             'resumed run draws what an uninterrupted one would, and a run may be resumed with or without the flag.  Not with '
                             '--embedding_prefix_cache, whose cache holds the frozen prefix\'s output for ONE image per frame; --embedding_prefix_once is '
                             'the compatible mode')
    parser.add_argument('--embedding_random_resized_crop', type=float, nargs=2, default=None, metavar=('LO', 'HI'),
                        help='with --train_embedding: every frame of a training step is replaced by torchvision\'s RandomResizedCrop(224, scale=(LO, HI), '
                             'ratio=(3/4, 4/3)) of the original frame - a rectangle whose area is uniform in [LO, HI] of the frame\'s and whose aspect ratio '
                             'is log-uniform in [3/4, 4/3], resized to 224 x 224 - instead of Resize(256) and the centre crop (MoCo\'s crop is 0.2 1; '
                             'evaluation keeps Resize(256) and the centre crop).  Default off.  The rectangles are a function of --run_id, the iteration and '
                             'the frame, so a resumed run draws what an uninterrupted one would, and a run may be resumed with or without the flag.  Composes '
                             'with --embedding_color_jitter.  Not with --embedding_random_crop (both choose the window), and not with '
                             '--embedding_prefix_cache, whose cache holds the frozen prefix\'s output for ONE window per frame; --embedding_prefix_once is '
                             'the compatible mode')
    parser.add_argument('--embedding_gaussian_blur', type=float, nargs=3, default=None, metavar=('P', 'LO', 'HI'),
                        help='with --train_embedding: with probability P a frame of a training step is blurred as torchvision\'s GaussianBlur(kernel_size=23, '
                             'sigma=(LO, HI)) blurs a uint8 tensor, sigma uniform in [LO, HI] - after the crop, the colour jitter and the grayscale, before '
                             '/ 255 and Normalize (MoCo v2\'s blur is 0.5 0.1 2.0; evaluation keeps the plain centre crop).  The kernel size is fixed at 23.  '
                             'Default off.  The draw is a function of --run_id, the iteration and the frame, so a resumed run draws what an uninterrupted '
                             'one would.  Composes with --embedding_random_grayscale, --embedding_random_crop or --embedding_random_resized_crop and '
                             '--embedding_color_jitter.  Not with --embedding_prefix_cache; --embedding_prefix_once is the compatible mode')
    parser.add_argument('--embedding_random_grayscale', type=float, default=None, metavar='P',
                        help='with --train_embedding: with probability P the three channels of a frame of a training step are replaced by its gray value, '
                             'torchvision\'s RandomGrayscale on a uint8 tensor - after the crop and the colour jitter, before the blur (MoCo v2\'s is 0.2; '
                             'evaluation keeps the plain centre crop).  Default off.  The draw is a function of --run_id, the iteration and the frame.  Not '
                             'with --embedding_prefix_cache; --embedding_prefix_once is the compatible mode')
    parser.add_argument('--batch_norm', action='store_true')
    # not in the reference (src/arguments.py): 5 = corner + centre windows per frame (BASELINE config 5 extension), 1 = CenterCrop
    parser.add_argument('--crops', type=int, default=1, choices=[1, 5])
    # Environment Settings.
    parser.add_argument('--env', type=str, default='HabitatImageNav-apartment_0')
    parser.add_argument('--num_input_frames', type=int, default=1)
    # General Settings.
    parser.add_argument('--xpid', default=None)
    parser.add_argument('--run_id', default=1, type=int)
    parser.add_argument('--seed', default=1, type=int)
    # Training settings.
    parser.add_argument('--total_frames', default=50000000, type=int)
    parser.add_argument('--batch_size', default=32, type=int)
    parser.add_argument('--unroll_length', default=100, type=int)
    parser.add_argument('--mp_start', default='spawn', type=str)
    parser.add_argument('--disable_cuda', action='store_true')
    # Optimizer settings.
    parser.add_argument('--learning_rate', default=0.0001, type=float)
    parser.add_argument('--alpha', default=0.99, type=float)
    parser.add_argument('--momentum', default=0, type=float)
    parser.add_argument('--epsilon', default=1e-5, type=float)
    parser.add_argument('--max_grad_norm', default=40., type=float)
    # save_embedded_obs.py:25-26
    parser.add_argument('--n_trajectories', type=int, default=-1)
    parser.add_argument('--source', type=str, default='png', choices=['png', 'pickle'])
    # MI355X additions (not in the reference)
    parser.add_argument('--compute_dtype', type=str, default=None, choices=[None, 'bf16', 'f16', 'f32', 'f32s'],
                        help='encoder storage/MFMA input type (default: $PVR_DTYPE or f16 = inside the 1e-3 parity bound; bf16 = wider range, 3e-3; '
                             'f32 = fp32 storage on the f32 MFMA, ~1e-6; f32s = the same on the 16-bit MFMA as exact split products, ResNet family)')
    parser.add_argument('--embed_batch', type=int, default=256, help='frames per encoder launch (the reference '
                        'pushes batch_size x n_frames = 64 per forward, save_embedded_obs.py:151-153)')
    parser.add_argument('--embed_block', type=int, default=0, help='observation rows a rank reads, embeds and appends to its shard file at a '
                        'time (bounds host memory for scenes of millions of frames); 0 = about 1 GiB of frames')
    parser.add_argument('--num_actions', type=int, default=3, help='size of the policy head when no simulator is attached (the reference '
                        'reads env.gym_env.action_space.n, main_bc_2.py:77; Habitat ImageNav without STOP has 3 actions, gym_wrappers.py:173). '
                        'The data is checked against it - it is never derived from the data')
    parser.add_argument('--autograd_step', action='store_true', help="run the reference's own training lines (loss.backward(), "
                        'clip_grad_norm_, torch.optim.RMSprop.step(): main_bc_2.py:206-227) through the autograd bridge instead of the fused step')
    parser.add_argument('--optimizer', type=str, default='rmsprop', choices=['rmsprop', 'adam'],
                        help="'rmsprop' is the reference's optimiser (main_bc_2.py:80-86); 'adam' is an extension")
    return parser


parser = make_parser()
