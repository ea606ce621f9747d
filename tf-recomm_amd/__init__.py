"""tf-recomm_amd: MI355X-native SVD matrix-factorisation training step.

One hot path of jilljenn/TF-recomm (ops.inference_svd + ops.optimization + the
svd_train_val.py minibatch step + dataio.ShuffleIterator) as hand-written gfx950 HIP
kernels behind the C-ABI of include/tfrecomm.h.  Import as ``import tfrecomm_amd``
(the directory name has a hyphen; ``tfrecomm_amd.py`` at the repo root aliases it).
"""
from . import _lib
from ._lib import TfrError, OutOfRangeError
from .engine import SvdModel, device_copy_rate, rated_matrix
from . import dataio, graph, ops, config, cats, adaptive_test, finetune
from .fm import FmModel
from .svdpp import SvdppModel
from . import svdpp
from .als import MangakiALS3
from .ials import ImplicitALS
from .itemknn import ItemKNN
from .userknn import UserKNN
from .rp3beta import WeightedItemKNN, RP3beta
from .ease import EASE
from .slim import SLIM
from .puresvd import PureSVD
from . import ranking, neighbours, bf16
from .ranking import ranking_metrics, evaluate_ranking

__all__ = ["SvdModel", "device_copy_rate", "rated_matrix", "TfrError", "OutOfRangeError", "_lib", "dataio", "graph", "ops", "config", "cats", "adaptive_test", "finetune",
           "FmModel", "SvdppModel", "svdpp", "MangakiALS3", "ImplicitALS", "ItemKNN", "UserKNN", "WeightedItemKNN", "RP3beta", "EASE", "SLIM", "PureSVD", "ranking", "ranking_metrics", "evaluate_ranking", "neighbours", "bf16"]
