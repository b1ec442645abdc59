"""The Keras callback protocol the reference's README uses (README.md:71-97)."""


class Callback(object):
    def __init__(self):
        self.model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass


class LearningRateScheduler(Callback):
    """tf.keras.callbacks.LearningRateScheduler(schedule): lr = schedule(epoch, lr) at epoch begin."""

    def __init__(self, schedule, verbose=0):
        super().__init__()
        self.schedule = schedule
        self.verbose = verbose

    def on_epoch_begin(self, epoch, logs=None):
        opt = self.model.optimizer
        if getattr(opt, "has_schedule", False):
            # Keras: "optimizer was created with a LearningRateSchedule object as its learning_rate: cannot set a value on it"
            raise TypeError("LearningRateScheduler: the optimizer's learning_rate is a %s schedule object, a value cannot be set on it "
                            "(as in Keras); compile with a numeric learning_rate to use this callback" % type(opt.learning_rate).__name__)
        lr = float(self.schedule(epoch, opt.learning_rate))
        opt.learning_rate = lr
        if self.verbose:
            print("Epoch %d: LearningRateScheduler setting learning rate to %g." % (epoch + 1, lr))

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs["lr"] = self.model.optimizer.learning_rate
