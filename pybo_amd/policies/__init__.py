"""Acquisition policies; the exported names match pybo.policies (`EI`, `PI`, `UCB`, `Thompson`), plus `MES`."""
from .simple import EI, PI, UCB, Thompson, MES

__all__ = ['EI', 'PI', 'UCB', 'Thompson', 'MES']
