"""Working memory that adds its gated input to what it holds.

Mirrors the reference's ``AdditiveInputGatedMemory`` (``sspslam/networks/workingmemory.py:12-80``, itself adapted from
``nengo.networks.InputGatedMemory``): ``mem`` is an ``EnsembleArray`` integrator (``mem.output -> mem.input`` through
``recurrent_synapse``, ``:35-40``) that accumulates ``gain * inputnet`` through ``difference_synapse`` (``:45-50``).
``gate`` (0 = take the input in, 1 = hold) inhibits the populations that compute the input directly on their neurons with
a weight of -10 (``:54-70``) - either the arrays of a list, through their ``add_neuron_input()`` nodes, or one
``ensemble.neurons`` - and ``reset`` (1 = forget) inhibits the memory's own neurons with -3 (``:73-79``).  On this stack
the neuron inputs of the arrays become drive columns of their array operators (``builder._lower_drive``).
"""
import numpy as np

from .. import frontend as nengo


class AdditiveInputGatedMemory(nengo.Network):
    def __init__(self, inputnet, inputnetneurons, n_neurons, dimensions, feedback=1.0, gain=1.0,
                 recurrent_synapse=0.1, difference_synapse=None, **kwargs):
        super().__init__()
        if difference_synapse is None:
            difference_synapse = recurrent_synapse
        with self:
            self.mem = nengo.EnsembleArray(n_neurons, dimensions, label="mem", **kwargs)
            nengo.Connection(self.mem.output, self.mem.input, transform=feedback, synapse=recurrent_synapse)
            nengo.Connection(inputnet, self.mem.input, transform=gain, synapse=difference_synapse)

            self.gate = nengo.Node(size_in=1)
            arrays = inputnetneurons if isinstance(inputnetneurons, list) else None
            for target in ([ea.add_neuron_input() for ea in arrays] if arrays is not None else [inputnetneurons]):
                nengo.Connection(self.gate, target, transform=-10.0 * np.ones((target.size_in, 1)), synapse=None)

            self.reset = nengo.Node(size_in=1)
            nengo.Connection(self.reset, self.mem.add_neuron_input(),
                             transform=-3.0 * np.ones((n_neurons * dimensions, 1)), synapse=None)
        self.output = self.mem.output
