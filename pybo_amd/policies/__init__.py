"""Acquisition policies; the exported names match pybo.policies (`EI`, `PI`, `UCB`, `Thompson`), plus `MES` and `KG`."""
from .simple import EI, PI, UCB, Thompson, MES, KG

__all__ = ['EI', 'PI', 'UCB', 'Thompson', 'MES', 'KG']
