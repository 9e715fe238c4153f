"""Acquisition policies; the exported names match pybo.policies (`EI`, `PI`, `UCB`, `Thompson`), plus `MES`, `KG`, `CEI` and `EHVI`."""
from .simple import EI, PI, UCB, Thompson, MES, KG, CEI, EHVI

__all__ = ['EI', 'PI', 'UCB', 'Thompson', 'MES', 'KG', 'CEI', 'EHVI']
