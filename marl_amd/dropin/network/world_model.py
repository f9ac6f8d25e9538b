"""`from network.world_model import Agent` (reference controller/share_params.py:5) resolves to the product classes.
TeammateModel and MessageGenerator (reference world_model.py:79-119) are never constructed by the reference and are not
built here."""
from marl_amd.network.world_model import WorldModel, Agent  # noqa: F401


class _NotBuilt:
    def __init__(self, *a, **k):
        raise NotImplementedError("%s (reference network/world_model.py) is outside this project: nothing in the reference "
                                  "constructs it" % type(self).__name__)


class TeammateModel(_NotBuilt):
    pass


class MessageGenerator(_NotBuilt):
    pass
