"""go_with_the_flows_amd -- MI355X-native discrete point-flow decoder (gfx950 HIP behind the reference's nn.Module API)."""
from .layers import SharedDot, Swish
from .flows import CondRealNVPFlow3D, CondRealNVPFlow3DTriple, WARP_PATTERNS
from .decoders import LocalCondRNVPDecoder
from .mixture import MixtureStack, flow_mixture_nll
from . import optim
from . import metrics
from . import render
from . import evaluation
from .encoders import PointNetCloudEncoder, FeatureEncoder, WeightsEncoder
from .prior import RealNVPFlow, RealNVPFlowCouple, GlobalRNVPDecoder, GaussianFlowNLL, GaussianEntropy
from .models import Local_Cond_RNVP_MC_Global_RNVP_VAE, Flow_Mixture_Model, Flow_Mixture_SVR_Model, Flow_Mixture_Loss, FlowMixtureNLL
from .resnet import ResNet, BasicBlock, resnet18
from .clouds import MeshStore, CloudStore, CloudTransform, DeviceCloudLoader, sample_clouds, sample_stored_clouds, make_state
from .images import ImageStore, ImageTransform, DeviceSVRLoader, transform_images
from .metrics import EvalFrame, clouds_to_eval_frame, chamfer_paired, paired_metrics
from .evaluation import (evaluate_generation, evaluate_autoencoding, evaluate_reconstruction, interpolate_clouds, upsample_clouds,
                         segment_clouds, part_agreement, reconstruction_figure, sweep_figure, segmentation_figure)
from .render import PALETTE, GROUND_TRUTH_RGB, view_matrix, fit_views, render_clouds, save_png
from ._lib import GwtfError

__all__ = ['SharedDot', 'Swish', 'CondRealNVPFlow3D', 'CondRealNVPFlow3DTriple', 'LocalCondRNVPDecoder',
           'WARP_PATTERNS', 'GwtfError', 'MixtureStack', 'flow_mixture_nll', 'optim', 'metrics', 'evaluation',
           'PointNetCloudEncoder', 'FeatureEncoder', 'WeightsEncoder', 'RealNVPFlow', 'RealNVPFlowCouple',
           'GlobalRNVPDecoder', 'GaussianFlowNLL', 'GaussianEntropy', 'Local_Cond_RNVP_MC_Global_RNVP_VAE',
           'Flow_Mixture_Model', 'Flow_Mixture_SVR_Model', 'Flow_Mixture_Loss', 'FlowMixtureNLL', 'ResNet', 'BasicBlock',
           'resnet18', 'MeshStore', 'CloudStore', 'CloudTransform', 'DeviceCloudLoader', 'sample_clouds', 'sample_stored_clouds', 'make_state',
           'ImageStore', 'ImageTransform', 'DeviceSVRLoader', 'transform_images', 'EvalFrame', 'clouds_to_eval_frame',
           'chamfer_paired', 'paired_metrics', 'evaluate_generation', 'evaluate_autoencoding', 'evaluate_reconstruction',
           'interpolate_clouds', 'upsample_clouds', 'segment_clouds', 'part_agreement', 'render', 'PALETTE', 'GROUND_TRUTH_RGB',
           'view_matrix', 'fit_views', 'render_clouds', 'save_png', 'reconstruction_figure', 'sweep_figure', 'segmentation_figure']
