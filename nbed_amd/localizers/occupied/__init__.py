"""Occupied localizer classes (mirror of nbed/localizers/occupied/__init__.py)."""

from .base import OccupiedLocalizer
from .spade import SPADELocalizer
from .jacobi import BOYSLocalizer, PMLocalizer
from .unsupported import IBOLocalizer

__all__ = ["BOYSLocalizer", "IBOLocalizer", "PMLocalizer", "SPADELocalizer", "OccupiedLocalizer"]
