"""The model registry of the reference (ggpm/opvnet.py:4-9): ``OPVNet.get_model(name)(args)``."""
from .property_vae import HierPropertyVAE, HierPropOptVAE, PropertyVAE, PropOptVAE


class OPVNet:
    MODEL_DICT = {
        'prop': PropertyVAE,
        'prop-opt': PropOptVAE,
        'hier-prop': HierPropertyVAE,
        'hier-prop-opt': HierPropOptVAE,
    }

    @staticmethod
    def get_model(name):
        return OPVNet.MODEL_DICT[name]
