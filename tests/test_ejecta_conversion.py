"""Argument checks of the device conversion objects (``nmma_amd/core/conversion.py``): they run without a device."""
import numpy as np
import pytest

from nmma_amd import _lib as L
from nmma_amd.core.conversion import EOSTableConverter, plan_mm_conversion

TABLE = (np.array([12.0, 11.8, 11.0]), np.array([1.0, 1.5, 2.1]), np.array([3000.0, 400.0, 10.0]))
NAMES = ["chirp_mass", "mass_ratio", "luminosity_distance", "alpha", "ratio_zeta"]
GRID = (np.array([1.0, 100.0]), np.array([1e-4, 0.02]))


def test_argument_checks_and_the_plan():
    with pytest.raises(NotImplementedError, match="Gaussian jet"):
        plan_mm_conversion(NAMES + ["alphaWing"], {}, [TABLE], GRID)
    with pytest.raises(NotImplementedError, match="Gaussian jet"):
        plan_mm_conversion(NAMES + ["thetaWing", "thetaCore"], {}, [TABLE], GRID)
    with pytest.raises(ValueError, match="EOS 1: the masses are not strictly ascending"):
        EOSTableConverter([TABLE, (TABLE[0], np.array([1.0, 2.1, 2.0]), TABLE[2])])
    with pytest.raises(ValueError, match="positive"):
        EOSTableConverter([(TABLE[0], TABLE[1], np.array([3000.0, 0.0, 10.0]))])
    plan = plan_mm_conversion(NAMES, {}, [TABLE], GRID)
    assert (plan["eos_mode"], plan["jet"], plan["mass_mode"], plan["redshift_mode"]) == (L.MM_EOS_SINGLE, L.MM_JET_TOPHAT, L.MM_CHIRP_MASS_RATIO, L.Z_GRID)
    assert plan["derived"] == list(L.MM_OUTPUTS)
    # a derived key that is itself sampled (or fixed) keeps its value: it is not among the columns the kernel writes
    plan = plan_mm_conversion(NAMES + ["EOS", "log10_mej_wind", "b", "alphaWing"], {"log10_E0": 50.0}, [TABLE, TABLE], GRID)
    assert (plan["eos_mode"], plan["jet"]) == (L.MM_EOS_TABLES, L.MM_JET_NONE)
    assert plan["derived"] == [k for k in L.MM_OUTPUTS if k not in ("log10_mej_wind", "log10_E0")]
    plan = plan_mm_conversion(["mass_1", "mass_2", "redshift", "lambda_1", "lambda_2", "alpha", "ratio_zeta", "b", "alphaWing"], {"TOV_mass": 2.2})
    assert (plan["eos_mode"], plan["jet"], plan["redshift_mode"]) == (L.MM_EOS_QUR, L.MM_JET_POWERLAW, L.Z_SLOT)
    assert plan["derived"] == ["log10_mej_dyn", "log10_mej_wind", "log10_mej", "log10_E0", "radius_1", "radius_2", "R_16"]
