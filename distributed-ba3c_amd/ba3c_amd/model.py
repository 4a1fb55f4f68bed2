"""The BA3C `Model(ModelDesc)` of OpenAIGym/train.py:138-330, bound to libba3c.

Same method names and input contract as the reference: `_get_input_vars` (train.py:144-151),
`_build_graph(inputs)` (train.py:274-327; is_training=False stops after the predictor
outputs, :302-304), `get_cost`, `get_gradient_processor` (train.py:329-330) and
`vars_for_save` (checkpoint keys).  `_build_graph` executes the fused HIP forward (+ loss
+ backward when training) on the current stream; the results are device tensors.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .engine import Ba3cEngine
from .model_desc import (ClipByGlobalNorm, InputVar, MapGradient, ModelDesc, clip_by_average_norm,
                         get_current_tower_context)

IMAGE_SIZE = (84, 84)     # train.py:92
FRAME_HISTORY = 4         # train.py:93
LOCAL_TIME_MAX = 5        # train.py:102
GAMMA = 0.99              # train.py:94

# the clipped-surrogate loss of one step (ba3c_amd.ppo; Ba3cTrainer.train_step's arguments)
PpoStep = namedtuple("PpoStep", ["rows", "clip", "vclip", "adv_from_row"])


class Model(ModelDesc):
    def __init__(self, num_actions, channels=1, fc_neurons=512, fc_splits=1,
                 replace_with_conv=True, ps=1, batch_size=128, max_batch=None, engine=None,
                 seed=0, conv_init="normal", fc_init="uniform", max_grad_norm=None):
        """channels: the reference's --channels (frames per history step; CHANNEL =
        FRAME_HISTORY*channels, train.py:95).  BASELINE's 84x84x4 input is channels=1.
        A new engine starts from the reference initialisers (--conv_init / --fc_init,
        initializers.py) drawn with `seed`; a caller-supplied engine keeps its variables.
        max_grad_norm: the clip of the whole gradient's norm (ba3c_amd.gradclip) in place of the
        reference's per-tensor clip_by_average_norm(g, 0.1); None: the reference's."""
        self.num_actions = num_actions
        self.channel = FRAME_HISTORY * channels
        self.batch_size = batch_size
        if engine is None:
            engine = Ba3cEngine(num_actions=num_actions, channels=self.channel,
                                fc_neurons=fc_neurons, fc_splits=fc_splits,
                                replace_with_conv=replace_with_conv, ps=ps,
                                max_batch=max_batch or max(batch_size, 16))
            engine.init_params(seed=seed, conv_init=conv_init, fc_init=fc_init)
        self.engine = engine
        self.entropy_beta = 0.01      # non-trainable var 'entropy_beta' (train.py:296-297)
        self.explore_factor = 1.0     # non-trainable var 'explore_factor' (train.py:294-295)
        self.vars_for_save = {n: n for n in self.engine.tensor_names}
        self.cost = None
        self.ratio = None             # the last PPO pass's per-sample rho (device, [B])
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._global_clip = None if max_grad_norm is None else ClipByGlobalNorm(max_grad_norm)

    def _get_input_vars(self):
        return [InputVar(torch.uint8, (None,) + IMAGE_SIZE + (self.channel,), "state"),
                InputVar(torch.int64, (None,), "action"),
                InputVar(torch.float32, (None,), "futurereward"),
                InputVar(torch.float32, (self.batch_size,), "global_step_from_predict"),
                InputVar(torch.float32, (None,), "init_R"),
                InputVar(torch.bool, (None,), "isOver")]

    def _build_graph(self, inputs, phase=0, ppo=None):
        """phase 1 / 2: the two halves of the training pass around the fc1 + heads gradient bucket
        (Ba3cTrainer's bucketed data-parallel step), 0: the whole pass.  ppo: a PpoStep, the
        pass's loss; None: the A3C loss."""
        state, action, futurereward = inputs[0], inputs[1], inputs[2]
        ctx = get_current_tower_context()
        is_training = True if ctx is None else ctx.is_training
        if not is_training:
            self.logits, self.logitsT, self.value = self.engine.forward(
                state, explore_factor=self.explore_factor)
            return
        self.delay = inputs[3] if len(inputs) > 3 else None
        if ppo is not None:
            sc = self.engine.train_grads_ppo(state, action, ppo.rows, ppo.clip,
                                             entropy_beta=self.entropy_beta, phase=phase,
                                             vclip=ppo.vclip, adv_from_row=ppo.adv_from_row)
            self.ratio = self.engine.ratio[:state.shape[0]]
        else:
            sc = self.engine.train_grads(state, action, futurereward,
                                         entropy_beta=self.entropy_beta, phase=phase)
        self.scalars = sc
        self.cost = sc[0]

    def get_gradient_processor(self):
        if self._global_clip is not None:
            return [self._global_clip]
        return [MapGradient(clip_by_average_norm(0.1))]

    def get_predict_func(self, input_names=("state",), output_names=("logitsT", "pred_value")):
        from .predict import OnlinePredictor
        return OnlinePredictor(self, input_names, output_names)

    def scalars_dict(self):
        vals = self.scalars.tolist()
        d = dict(zip(_lib.SCALAR_NAMES, vals))
        d["active_relus"] = int(round(d["active_relus"]))
        return d
