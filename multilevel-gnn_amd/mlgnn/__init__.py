"""Host side of libmlgnn.so: loader, graph container, autograd bindings, data-parallel helper.

There is no CPU fallback.  Every op in this package launches a HIP kernel through the C ABI
declared in ``include/mlgnn.h``; importing :mod:`mlgnn._lib` raises if the shared library has not
been built (``python __graft_entry__.py`` or ``python multilevel-gnn_amd/build_native.py``).
"""
from .gat import gat_aggregate  # noqa: F401
from .graph import CSRGraph, as_graph  # noqa: F401
from .mha import mha_attention  # noqa: F401
from .conv import PathConv2d, conv2d, conv2d_supported  # noqa: F401
from .pool_flatten import module_pool_flatten, pool_flatten, pool_flatten_supported  # noqa: F401
from .mmd import mmd_per_pathway, mmd_supported  # noqa: F401
from .decoder import decoder_supported, pathway_decoders  # noqa: F401
from .vq import vector_quantize, vq_supported  # noqa: F401
from .latent import vae_latent, vae_latent_supported  # noqa: F401
from .criterion import TrainCriterion, criterion_supported, train_criterion  # noqa: F401
from .pathway_conv import PathwayTopology, pathway_aggregate, pathway_conv_supported  # noqa: F401
from .mutual_info import mutual_info_classif, mutual_info_supported, tree_path  # noqa: F401
from .mutual_info import (mutual_info_cc, mutual_info_regression, mutual_info_regression_supported,  # noqa: F401
                          prepare_regression)
from .pca import fold_pca, fold_pca_scores, pathway_pca, pathway_pca_supported  # noqa: F401
from .reorder import fold_reorder, pathway_order, pathway_order_host, pathway_order_supported  # noqa: F401
from .metrics import (EvalBuffer, EvalResult, binary_metrics, binary_metrics_host,  # noqa: F401
                      eval_metrics_supported)
from .survival import (ScreenResult, logrank_screen, logrank_screen_host, survival_screen_supported,  # noqa: F401
                       survival_table)
from .explain import explain_cohort, integrated_gradients, pathway_scores  # noqa: F401
from .edge_select import edge_select, edge_select_supported, pair_mutual_info  # noqa: F401
from .edge_select_reg import (edge_select_regression, edge_select_regression_supported,  # noqa: F401
                              pair_mutual_info_regression)
from .kraskov import edge_select_knn, kraskov_mi, kraskov_mi_host, kraskov_mi_supported  # noqa: F401
from .ops import (LowRankEdge, RankOneEdge, TableEdge, edge_type_embedding, gen_aggregate, share_edge_gradient,  # noqa: F401
                  weighted_mean_aggregate)
