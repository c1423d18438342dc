"""Model registry with the reference's surface: ``from models import get_model`` (reference
``models/__init__.py:11-24``): all nine names the reference registers.  'multiomix' is the multi-omics model
(``deepergcn_virtual_node.py``: three DeeperGCN_Vnode encoders with a PathwayConv behind every gene convolution past the
first)."""
from .deepergcn import DeeperGCN
from .deepergcn_virtual_node import DeeperGCN_Vnode, MultiOmixGCN  # noqa: F401
from .multilevel_gnn import MultilevelGNN
from .pathcnn import PathCNN
from .multilevel_gnn_seq import MultilevelGNNSeq, PathwayHeadSeq  # noqa: F401
from .vae import VAE, VQ_VAE, AutoEncoder, VectorQuantizer  # noqa: F401
from .diff_pooling import DiffPool, DiffPoolLayer, SAGEConvolutions  # noqa: F401

MODELS = {
    'deepergcn': DeeperGCN,
    'multilevel_gnn': MultilevelGNN,
    'multilevel_gnn_seq': MultilevelGNNSeq,
    'vae': VAE,
    'mmd_vae': VAE,
    'vq_vae': VQ_VAE,
    'autoencoder': AutoEncoder,
    'pathcnn': PathCNN,
    'multiomix': MultiOmixGCN,
}


def get_model(model_name):
    return MODELS[model_name]
