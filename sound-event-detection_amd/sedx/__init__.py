"""sedx — MI355X-native inference path of yazdayy/sound-event-detection.

Public surface (mirrors the reference's hot-path API):
  sedx.models      the seven 9-layer models: Cnn_9layers_Gru_FrameAtt,
                   Cnn_9layers_Transformer_FrameAtt, Cnn_9layers_FrameMax,
                   Cnn_9layers_FrameAvg, Cnn_9layers_FrameAtt, Cnn_9layers_Gru_FrameAvg,
                   Cnn_9layers_Transformer_FrameAvg (+ helpers), the Conformer models
                   Cnn_9layers_Conformer_FrameAtt / _FrameAvg and Cnn_14layers_Conformer_FrameAtt,
                   the 14-layer, Cnn14 and VGGish models
  sedx.inference   predict_windows, inference_prob, gamma_features, events_from_framewise
  sedx.calibrate   optimize_sed_thresholds, segment_counts, segment_metrics, segment_targets
  sedx.evaluate    Evaluator, average_precision, sed_average_precision, ranked_counts,
                   strong_targets, weak_targets
  sedx.distributed clip sharding + framewise gather over RCCL
  sedx.synth       seeded synthetic weights / waveforms (bench, tests)
"""
__version__ = '0.1.0'

_CALIBRATE = ('optimize_sed_thresholds', 'segment_counts', 'segment_metrics', 'segment_targets')
_EVALUATE = ('Evaluator', 'average_precision', 'sed_average_precision', 'ranked_counts', 'strong_targets',
             'weak_targets')


def __getattr__(name):
    # the calibration and evaluation entry points, importable from the package
    # itself (resolved on first use: importing sedx stays free of torch)
    if name in _CALIBRATE:
        from . import calibrate
        return getattr(calibrate, name)
    if name in _EVALUATE:
        from . import evaluate
        return getattr(evaluate, name)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
