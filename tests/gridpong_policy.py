"""The GridPong tests' scripted policy, shared by the CPU and the GPU tests."""
import numpy as np

from ba3c_amd import gridpong as K


def tracking_actions(game, rs=None):
    """Meet the ball with the paddle's top edge (a steep return), wait at the centre between
    points: actions int64 [E] for the rows of `game`."""
    tgt = np.where(game[:, K.SERVE] > 0, K.PY0, game[:, K.BY] >> K.SUB)
    py = game[:, K.PY]
    return np.where(py > tgt, K.UP, np.where(py < tgt, K.DOWN, K.FIRE)).astype(np.int64)
