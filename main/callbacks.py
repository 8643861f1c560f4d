"""The image-logging callback of the training loop at the drop-in boundary (reference: main/callbacks.py, ImageLogger 15-102).

A plain class with the reference's constructor arguments and hook signatures, no Lightning: whatever drives the loop calls
on_train_batch_end / on_validation_batch_end(trainer, pl_module, outputs, batch, batch_idx) after a batch.  Every `batch_frequency`
training batches (every 5 validation batches) it switches the module to eval(), calls pl_module.log_images(batch, split=...,
**log_images_kwargs), writes what comes back with utils.save_video (log_local) under <save_dir>/images/<split>/ and switches back
to train().  Only to_local=True is built (the other branch writes to a TensorBoard experiment).  Lightning's bookkeeping attributes
(current_epoch, global_step, global_rank) are read from the module when it has them and count as 0 otherwise; only rank 0 logs."""
import logging
import os

import torch

from utils.save_video import log_local, prepare_to_log

mainlogger = logging.getLogger("mainlogger")


class ImageLogger:
    def __init__(self, batch_frequency, max_images=8, clamp=True, rescale=True, save_dir=None, to_local=False, log_images_kwargs=None):
        if not to_local:
            raise NotImplementedError("ImageLogger(to_local=False) logs to a TensorBoard experiment, which is not part of this package: "
                                      "use to_local=True")
        self.rescale = rescale
        self.batch_freq = batch_frequency
        self.max_images = max_images
        self.to_local = to_local
        self.clamp = clamp
        self.log_images_kwargs = log_images_kwargs if log_images_kwargs else {}
        self.save_dir = os.path.join(save_dir, "images")
        os.makedirs(os.path.join(self.save_dir, "train"), exist_ok=True)
        os.makedirs(os.path.join(self.save_dir, "val"), exist_ok=True)

    def log_batch_imgs(self, pl_module, batch, batch_idx, split="train"):
        """generate images, then save them"""
        if getattr(pl_module, "global_rank", 0) != 0:
            return
        skip_freq = self.batch_freq if split == "train" else 5
        if (batch_idx + 1) % skip_freq != 0:
            return
        is_train = pl_module.training
        if is_train:
            pl_module.eval()
        try:
            with torch.no_grad():
                batch_logs = pl_module.log_images(batch, split=split, **self.log_images_kwargs)
            batch_logs = prepare_to_log(batch_logs, self.max_images, self.clamp)
            filename = "ep{}_idx{}_rank{}".format(getattr(pl_module, "current_epoch", 0), batch_idx, getattr(pl_module, "global_rank", 0))
            mainlogger.info("Log [%s] batch <%s> to local ..." % (split, filename))
            filename = "gs{}_".format(getattr(pl_module, "global_step", 0)) + filename
            log_local(batch_logs, os.path.join(self.save_dir, split), filename, save_fps=10)
            mainlogger.info("Finish!")
        finally:
            if is_train:
                pl_module.train()

    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, dataloader_idx=None):
        if self.batch_freq != -1 and pl_module.logdir:
            self.log_batch_imgs(pl_module, batch, batch_idx, split="train")

    def on_validation_batch_end(self, trainer, pl_module, outputs, batch, batch_idx, dataloader_idx=None):
        if self.batch_freq != -1 and pl_module.logdir:
            self.log_batch_imgs(pl_module, batch, batch_idx, split="val")
