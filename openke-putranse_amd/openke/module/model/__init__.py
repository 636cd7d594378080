from __future__ import absolute_import, division, print_function

from .Model import Model
from .TransE import TransE
from .TransH import TransH
from .TransD import TransD
from .RotatE import RotatE
from .DistMult import DistMult
from .ComplEx import ComplEx

__all__ = ['Model', 'TransE', 'TransH', 'TransD', 'RotatE', 'DistMult', 'ComplEx']
