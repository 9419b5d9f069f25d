"""One kspace.CrystalTables per crystal per call: the spin-orbit forward (9 assembly launches per crystal) and backward (9 launches + 8 adjoints) on the
two-crystal batch of tests/kspace_tables_checks.py build the tables, and sort the edges by atom pair, once per crystal."""
import pytest

from tests import kspace_tables_checks as KC

pytestmark = pytest.mark.gpu


def test_spin_orbit_step_builds_the_tables_once_per_crystal(monkeypatch):
    KC.check_built_once("cuda", monkeypatch)
