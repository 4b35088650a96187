from .model import FlavaKGC, MKGformerKGC, ViltKGC, VisualBertKGC
from .modeling_unimo import UnimoForMaskedLM
from .modeling_flava import FlavaForMaskedLM, flava_config
from .modeling_vilt import ViltForMaskedLM, draw_patch_order, vilt_config
from .modeling_visual_bert import VisualBertForMaskedLM, visual_bert_config
from .configs import TextConfig, VisionConfig

__all__ = ["MKGformerKGC", "FlavaKGC", "ViltKGC", "VisualBertKGC", "VisualBertForMaskedLM", "visual_bert_config", "ViltForMaskedLM", "vilt_config", "draw_patch_order", "UnimoForMaskedLM", "FlavaForMaskedLM", "flava_config", "TextConfig", "VisionConfig"]
