"""Host-side mirror of Elliot's plugin surface for the latent-factor path."""
from .base_recommender_model import BaseRecommenderModel, init_charger
from .recommender_utils_mixin import RecMixin
from .latent_factor_models.BPRMF_batch.BPRMF_batch import BPRMF_batch
from .latent_factor_models.BPRMF.BPRMF import BPRMF
from .latent_factor_models.MF.matrix_factorization import MF
from .latent_factor_models.PMF.probabilistic_matrix_factorization import PMF
from .latent_factor_models.FunkSVD.funk_svd import FunkSVD
from .latent_factor_models.LogisticMF.logistic_matrix_factorization import LMF, LogisticMatrixFactorization
from .latent_factor_models.CML.CML import CML
from .latent_factor_models.MF2020.MF import MF2020
from .graph_based.lightgcn.LightGCN import LightGCN
from .graph_based.ngcf.NGCF import NGCF
from .graph_based.RP3beta.rp3beta import RP3beta
from .generic.Proxy.Proxy import ProxyRecommender
from .autoencoders.vae.multi_vae import MultiVAE
from .autoencoders.dae.multi_dae import MultiDAE
from .neural.NeuMF.neural_matrix_factorization import NeuMF
from .neural.GeneralizedMF.generalized_matrix_factorization import GMF
from .neural.ItemAutoRec.itemautorec import ItemAutoRec
from .neural.UserAutoRec.userautorec import UserAutoRec
from .knn.item_knn.item_knn import ItemKNN
from .knn.user_knn.user_knn import UserKNN
from .knn.attribute_item_knn.attribute_item_knn import AttributeItemKNN
from .knn.attribute_user_knn.attribute_user_knn import AttributeUserKNN
from .content_based.VSM.vector_space_model import VSM
from .knowledge_aware.kaHFM.kahfm import KaHFM
from .latent_factor_models.iALS.iALS import iALS
from .latent_factor_models.WRMF.wrmf import WRMF
from .autoencoders.EASE_R.ease_r import EASER
from .latent_factor_models.Slim.slim import Slim
from .latent_factor_models.PureSVD.pure_svd import PureSVD
from .algebric.slope_one.slope_one import SlopeOne
from .latent_factor_models.BPRSlim.bprslim import BPRSlim
from .adversarial.AMF.AMF import AMF
from .visual_recommenders.VBPR.VBPR import VBPR

__all__ = ["BaseRecommenderModel", "init_charger", "RecMixin", "BPRMF_batch", "BPRMF", "MultiVAE", "MultiDAE", "NeuMF", "GMF",
           "MF", "PMF", "FunkSVD", "LogisticMatrixFactorization", "LMF", "CML", "MF2020", "LightGCN", "NGCF", "ProxyRecommender",
           "ItemKNN", "UserKNN", "iALS", "WRMF", "EASER", "RP3beta", "Slim", "PureSVD",
           "AttributeItemKNN", "AttributeUserKNN", "VSM", "KaHFM", "SlopeOne", "BPRSlim", "ItemAutoRec", "UserAutoRec", "AMF",
           "VBPR"]
