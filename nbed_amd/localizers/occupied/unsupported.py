"""Names the reference exports whose algorithms are not built here.

IBO localisation (nbed/localizers/occupied/pyscf.py:382-438) needs intrinsic atomic orbitals built on PySCF's
MINAO basis data.  The class stays importable so that code written against ``nbed.localizers`` loads, and fails
loudly when instantiated.  Pipek-Mezey and Boys are in ``jacobi.py``.
"""

from __future__ import annotations

from .base import OccupiedLocalizer


class _Unsupported(OccupiedLocalizer):
    _name = "this"

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(
            f"{self._name} localisation is not part of the MI355X hot path (SPADE, PM and Boys are); "
            "use localization='spade', 'pm' or 'boys'."
        )

    def _localize_spin(self, c_matrix, occupancy, n_mo_overwrite=None):  # pragma: no cover
        raise NotImplementedError


class IBOLocalizer(_Unsupported):
    _name = "IBO"
