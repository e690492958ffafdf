"""trackmpnn_amd: MI355X-native (gfx950) implementation of the TrackMPNN message-passing hot path.

    from trackmpnn_amd import TrackMPNN          # drop-in for reference models/track_mpnn.py
"""
from .graph import (CallPlan, DeviceGraph, FrameGraph, device_graph_from_adjacency, WindowBuilder, batch_windows, concat_static_graphs, dense_static_graph,
                    graph_from_adjacency, graph_from_edges, plan_single, synth_window)
from .capture import CapturedWindow
from .chunks import ChunkSampler, DetectionStore, DrawnChunks, FramePlan, HostDraw, draw_chunks_host, make_chunks
from .frames import FramePrep, FrameStore, prep_host, resize_coeffs, resize_host
from .labeling import (BDD_RULES, KITTI_RULES, DetectionLabeler, LabelRules, label_detections_host, label_frame_host,
                       label_overlaps_host, synth_label_sequence)
from .loss import (CELoss, FocalLoss, classification_counts, classification_counts_windows, create_targets,
                   train_losses_windows)
from .loops import (VisInference, VisTraining, infer_dataset, infer_store, train_chunk, train_chunks, train_epoch, validate,
                    validate_store)
from .seqfeat import SequenceFeatures, SequenceSample, listed_features_host, sequence_features_host, sequence_vis_host
from .results import (BDD_RESULT_RULES, KITTI_RESULT_RULES, ResultRules, TrackResults, bdd_document_host, kitti_lines_host,
                      results_host, synth_result_sequence)
from .monitor import AttentionMonitor, TrainMonitor, ValMonitor, att_hist_host, val_counts_host, val_f1_host
from .mapeval import MapEvaluator, MapStore, map_best_host, map_host, synth_map_sequence
from .hota import HotaEvaluator, hota_host, hota_overall, hota_sim_host
from .evalprep import (KITTI_CAR, KITTI_PEDESTRIAN, EvalPrep, PrepRules, evalprep_frame_host, evalprep_host, evalprep_ioa_host,
                       synth_prep_sequence)
from .moteval import MotEvaluator, MotStore, mot_dist_host, mot_events_host, mot_overall, mot_summary_host
from .online import FeatureSpec, OnlineTracker, OnlineVis, online_features_host
from .optim import BucketAdam
from .track_mpnn import SparseAttention, TrackMPNN
from .tracking import TrackGraph
from .vishead import VisHead, vis_centres_host, vis_head_host, vis_pixels_host
from .embedloss import EmbeddingLoss, embedding_loss_host
from .espnet import EspCentres, EspEmbedNet, EspTrainNet, espnet_centres_host, espnet_decoder_grads_host, espnet_host
from .train_batch import AllChunksSkipped, LossWindows, TrainBatch, build_train_batch, build_train_batch_device

__all__ = ['TrackMPNN', 'CapturedWindow', 'TrackGraph', 'SparseAttention', 'create_targets', 'CELoss', 'FocalLoss', 'FrameGraph', 'CallPlan', 'graph_from_adjacency', 'graph_from_edges',
           'plan_single', 'DeviceGraph', 'device_graph_from_adjacency', 'WindowBuilder', 'batch_windows', 'synth_window', 'dense_static_graph', 'concat_static_graphs',
           'train_losses_windows', 'train_chunk', 'train_chunks', 'TrainBatch', 'LossWindows', 'build_train_batch',
           'build_train_batch_device', 'classification_counts', 'classification_counts_windows', 'TrainMonitor', 'BucketAdam',
           'make_chunks', 'DetectionStore', 'ChunkSampler', 'DrawnChunks', 'draw_chunks_host', 'train_epoch', 'AllChunksSkipped',
           'OnlineTracker', 'FeatureSpec', 'online_features_host', 'MotEvaluator', 'MotStore', 'mot_events_host', 'mot_summary_host', 'mot_dist_host',
           'mot_overall', 'HotaEvaluator', 'hota_host', 'hota_overall', 'hota_sim_host', 'validate', 'MapEvaluator', 'MapStore', 'map_host', 'map_best_host', 'synth_map_sequence',
           'ValMonitor', 'val_counts_host', 'val_f1_host', 'AttentionMonitor', 'att_hist_host', 'DetectionLabeler', 'LabelRules', 'KITTI_RULES', 'BDD_RULES',
           'label_frame_host', 'label_detections_host', 'label_overlaps_host', 'synth_label_sequence', 'VisHead', 'vis_centres_host',
           'vis_pixels_host', 'vis_head_host', 'FramePlan', 'HostDraw', 'FrameStore', 'VisTraining',
           'FramePrep', 'OnlineVis', 'resize_coeffs', 'resize_host', 'prep_host', 'infer_dataset', 'ResultRules',
           'KITTI_RESULT_RULES', 'BDD_RESULT_RULES', 'TrackResults', 'results_host', 'kitti_lines_host', 'bdd_document_host',
           'synth_result_sequence', 'EvalPrep', 'PrepRules', 'KITTI_CAR', 'KITTI_PEDESTRIAN', 'evalprep_frame_host', 'evalprep_host',
           'evalprep_ioa_host', 'synth_prep_sequence', 'SequenceFeatures', 'SequenceSample', 'sequence_features_host',
           'sequence_vis_host', 'listed_features_host', 'VisInference', 'validate_store', 'infer_store', 'EmbeddingLoss',
           'embedding_loss_host', 'EspEmbedNet', 'espnet_host', 'EspCentres', 'espnet_centres_host', 'EspTrainNet',
           'espnet_decoder_grads_host']
