"""Operator classes selected by name from the CLI, as in MarT/models/model.py:7-11 (``add_to_argparse`` comes from HipMaskedLM)."""
from .modeling_flava import FlavaForMaskedLM
from .modeling_unimo import UnimoForMaskedLM
from .modeling_vilt import ViltForMaskedLM
from .modeling_visual_bert import VisualBertForMaskedLM


class MKGformerKGC(UnimoForMaskedLM):
    pass


class FlavaKGC(FlavaForMaskedLM):
    """MarT/models/model.py:31."""


class ViltKGC(ViltForMaskedLM):
    """MarT/models/model.py ViltKGC (fine-tune only: the reference cannot run the MarKG pre-train step with ViLT)."""


class VisualBertKGC(VisualBertForMaskedLM):
    """MarT/models/model.py VisualBertKGC (fine-tune only: the reference cannot run the MarKG pre-train step without sep_idx)."""
