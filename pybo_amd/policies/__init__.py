"""Acquisition policies; the exported names match pybo.policies (`EI`, `PI`, `UCB`, `Thompson`), plus `MES`, `KG` and `CEI`."""
from .simple import EI, PI, UCB, Thompson, MES, KG, CEI

__all__ = ['EI', 'PI', 'UCB', 'Thompson', 'MES', 'KG', 'CEI']
