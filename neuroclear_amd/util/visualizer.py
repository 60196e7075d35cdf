"""Training progress views (reference: util/visualizer.py:88-287), without tensorboard / matplotlib / tifffile, none of which exists on
this image: the arrays the reference hands to its figures are written as plain files instead.

    <checkpoints_dir>/<name>/loss_log.txt                              header line per run, one line per --print_freq
    <checkpoints_dir>/<name>/web/images/iter_<n>_<label>_<key>.tif     the three centre slices and three maximum projections of every visual
                                                                       (key: slice_xy, slice_xz, slice_yz, mip_xy, mip_xz, mip_yz), 2-D uint8
    <checkpoints_dir>/<name>/web/images/iter_<n>_<label>_hist.npy      --display_histogram: counts of the 256 uint8 values, int64[256]
    <checkpoints_dir>/<name>/web/images/<n>_<label>.tif                tensor2im(image[0], uint8) of the whole visual (the reference's name)

The arrays come from HIP kernels (ops.progress_views / ops.tensor2im: csrc/views.hip); this class only names and writes files.  --no_html
turns off everything under web/; the loss log stays."""
import os
import time

import numpy as np

from .. import ops
from . import tiff


class Visualizer:
    def __init__(self, opt):
        self.opt = opt
        self.use_html = opt.isTrain and not opt.no_html
        self.name = opt.name
        self.display_histogram = opt.display_histogram
        self.saved = False
        if self.use_html:
            self.web_dir = os.path.join(opt.checkpoints_dir, opt.name, 'web')
            self.img_dir = os.path.join(self.web_dir, 'images')
            print('create web directory %s...' % self.web_dir)
            os.makedirs(self.img_dir, exist_ok=True)
        os.makedirs(os.path.join(opt.checkpoints_dir, opt.name), exist_ok=True)
        self.log_name = os.path.join(opt.checkpoints_dir, opt.name, 'loss_log.txt')
        with open(self.log_name, 'a') as log_file:
            log_file.write('================ Training Loss (%s) ================\n' % time.strftime('%c'))

    def reset(self):
        self.saved = False

    def display_model_hyperparameters(self):
        """tensorboard only in the reference (visualizer.py:233-239): writes nothing."""

    def plot_current_losses(self, plot_count, losses, is_epoch=False):
        """tensorboard only in the reference (visualizer.py:256-268): writes nothing."""

    def display_current_results(self, visuals, total_iters):
        """visualizer.py:128-201: per visual, the six arrays of its two figures."""
        if not self.use_html:
            return
        for label, image in visuals.items():
            views = ops.progress_views(image)
            for key in ops.VIEW_KEYS:
                tiff.imsave(os.path.join(self.img_dir, 'iter_%d_%s_%s.tif' % (total_iters, label, key)), views[key])

    def display_current_histogram(self, visuals, total_iters):
        """visualizer.py:241-244 (add_histogram of image[0][0]): here the counts of its uint8 values."""
        if not (self.use_html and self.display_histogram):
            return
        for label, image in visuals.items():
            np.save(os.path.join(self.img_dir, 'iter_%d_%s_hist.npy' % (total_iters, label)), ops.progress_views(image)['hist'])

    def save_current_visuals(self, visuals, total_iters):
        """visualizer.py:250-254."""
        if not self.use_html:
            return
        for label, image in visuals.items():
            img_np = ops.tensor2im(image[0], np.uint8)
            tiff.imsave(os.path.join(self.img_dir, str(total_iters) + '_' + str(label) + '.tif'), img_np.reshape((-1,) + img_np.shape[-2:]))  # [C, D, H, W] -> pages

    def print_current_losses(self, epoch, epoch_progress, losses, t_comp, t_data):
        """visualizer.py:270-287: the same message, printed and appended to loss_log.txt."""
        message = '(epoch: %d, epoch_progress: %d%%, iter time: %.3f, data load time: %.3f) ' % (epoch, epoch_progress, t_comp, t_data)
        for k, v in losses.items():
            message += '%s: %.3f ' % (k, v)
        print(message, flush=True)
        with open(self.log_name, 'a') as log_file:
            log_file.write('%s\n' % message)
