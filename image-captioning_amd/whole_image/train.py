"""image captioning/train.py: train() with the reference's ModelCheckpoint(monitor='loss', save_best_only=True); no TensorBoard."""
import os

from .model import create_model
from .pipeline import generate_config, train_generator


class BestCheckpoint(object):
    """keras.callbacks.ModelCheckpoint(filepath, monitor='loss', save_best_only=True, mode='min'): whole-model saving is weights
    saving here (Keras-layout HDF5 under the reference's layer names); an epoch whose monitored value did not improve writes nothing."""

    def __init__(self, filepath, monitor='loss', verbose=0, save_best_only=True, mode='min'):
        if mode not in ('min', 'max'):
            raise ValueError("mode must be 'min' or 'max', got %r" % (mode,))
        self.filepath, self.monitor, self.verbose, self.save_best_only = filepath, monitor, verbose, save_best_only
        self.sign = 1.0 if mode == 'min' else -1.0
        self.best = float("inf")

    def on_epoch_end(self, model, epoch, logs):
        current = logs.get(self.monitor)
        if self.save_best_only:
            if current is None or not self.sign * current < self.best:
                if self.verbose:
                    print("Epoch %05d: %s did not improve" % (epoch + 1, self.monitor))
                return
            self.best = self.sign * current
        path = self.filepath.format(epoch=epoch + 1, **logs)
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        model.save_weights(path)
        if self.verbose:
            print("Epoch %05d: %s improved to %.5f, saving model to %s" % (epoch + 1, self.monitor, current, path))


def train(batch_size=128, epochs=100, data_dir="../dataset/", weights_path=None, mode="train", model=None, dataset='flickr8k',
          steps_per_epoch=200, checkpoint="image captioning/model/weights-{epoch:02d}.hdf5", device_resident=True, load_image=None,
          feature_cache=None, verbose=1):
    """train.train: model = the FEATURE model (feature_generation's load_model()), as in the reference; the captioner is created from
    generate_config.  steps_per_epoch is the reference's fixed 200.  Returns (captioner, history)."""
    config_dict = generate_config(data_dir=data_dir, mode=mode, dataset=dataset)
    config_dict['batch_size'] = batch_size
    captioner = create_model(config_dict=config_dict)
    generator = train_generator(config_dict=config_dict, data_dir=data_dir, model=model, dataset=dataset, device_resident=device_resident,
                                load_image=load_image, feature_cache=feature_cache, device=captioner.device)
    if weights_path:
        captioner.load_weights(weights_path)
    callbacks = [BestCheckpoint(filepath=checkpoint, monitor='loss', verbose=verbose, save_best_only=True, mode='min')]
    history = captioner.fit_generator(generator=generator, steps_per_epoch=steps_per_epoch, epochs=epochs, verbose=verbose, callbacks=callbacks)
    return captioner, history
