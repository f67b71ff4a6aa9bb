"""``nmma_amd.em``: light-curve models, likelihoods, systematics (mirrors ``nmma.em``).  The power-law flux models are exported here
under both of their names; everything else is imported from its module."""
from .model import HostGalaxyLightCurveModel, PowerLawFluxLightCurveModel  # noqa: F401

__all__ = ["HostGalaxyLightCurveModel", "PowerLawFluxLightCurveModel"]
