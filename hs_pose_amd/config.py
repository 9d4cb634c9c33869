"""Stand-in for the reference's global absl ``FLAGS`` object (config/config.py:6-125).

Only the flags the hot path reads are defined (names and defaults as in the reference); modules read
them at construction and at forward time exactly where the reference does (FaceRecon.py:15-16,32-37,
114; PoseNet9D.py:27; PoseR.py:13-14; PoseTs.py:15-16).  Plain attribute bag: ``FLAGS.train = 0``
before constructing a model gives the eval-mode module set, like evaluation/evaluate.py:39.
"""


class _Flags:
    _defaults = dict(
        obj_c=6,              # config.py:6   number of categories
        feat_c_R=1286,        # config.py:31  input channels of the rotation heads
        R_c=4,                # config.py:32
        feat_c_ts=1289,       # config.py:33
        Ts_c=6,               # config.py:34
        feat_face=768,        # config.py:35
        face_recon_c=6 * 5,   # config.py:37
        img_size=256,         # config.py:19  side of the instance crop
        gcn_sup_num=7,        # config.py:39  support directions S
        gcn_n_num=20,         # config.py:40  neighbours k
        random_points=1028,   # config.py:43
        sample_method='basic',  # config.py:44
        train=1,              # config.py:48
        batch_size=16,        # config.py:55
        DZI_PAD_SCALE=1.5, DZI_TYPE='uniform', DZI_SCALE_RATIO=0.25, DZI_SHIFT_RATIO=0.25,   # config.py:13-16  the crop window's draws
        roi_mask_pro=0.5,     # config.py:23  share of the items whose cropped mask defor_2D perturbs
        roi_mask_r=3,         # config.py:22  defor_2D's iteration count -- which the reference's call never applies: it lands in
                              # cv2.erode's dst argument and ONE iteration runs (pc_sample.train_batch_to_pcl: mask_iters=1)
        aug_pc_pro=0.2, aug_pc_r=0.2, aug_rt_pro=0.3, aug_bb_pro=0.3, aug_bc_pro=0.3,   # config.py:24-28
        fsnet_loss_type='l1',                                                          # config.py:64
        rot_1_w=8.0, rot_2_w=8.0, rot_regular=4.0, tran_w=8.0, size_w=8.0, recon_w=8.0, r_con_w=1.0,   # config.py:66-72
        recon_n_w=3.0, recon_d_w=3.0, recon_v_w=1.0, recon_s_w=0.3, recon_f_w=1.0,      # config.py:74-78
        recon_bb_r_w=1.0, recon_bb_t_w=1.0, recon_bb_s_w=1.0, recon_bb_self_w=1.0,      # config.py:79-82
        geo_p_w=1.0, geo_s_w=10.0, geo_f_w=0.1,                                         # config.py:87-89
        prop_pm_w=2.0, prop_sym_w=1.0, prop_r_reg_w=1.0,                                # config.py:91-93
        lr=1e-4,              # config.py:96
        lr_pose=1.0,          # config.py:98
        pool_sampler='random',  # (not in the reference) Pool_layer's down-sampler: 'random' -- the reference's randperm slice --
                                # or 'fps' -- per-cloud farthest-point sampling on the device (gcn3d.Pool_layer)
        pc_sampler='host',      # (not in the reference) who draws the rows an instance cloud keeps (pc_sample.py): 'host' -- the
                                # reference's draws on numpy's global generator --, 'device' -- a keyed counter-based draw
                                # inside the front end (pc_sample.DeviceSampler), no count copy and no sync -- or 'fps' -- no
                                # draw: farthest-point picks over each instance's back-projected candidates (hsp_fps_ids), the
                                # frame front end only (frame_to_pcl, frame_to_pcl_device, frame.FramePipeline); PC_sample,
                                # depth_to_pcl and the training front end raise under it.  DESIGN.md section 8i
        step_draws='host',      # (not in the reference) who makes the draws of a forward or a replay -- the Pool_layers' kept
                                # rows, the augmentation's uniforms and jitter, the training loader's DZI windows: 'host' -- the
                                # reference's draws on torch's and numpy's generators, uploaded before a replay -- or 'device' --
                                # keyed draws inside the forward / the captured body (pc_sample.resolve_draws; include/hsp.h:
                                # "keyed draws of a step"): the same distributions, not the same draws, no host generator touched
        reproducible=False,     # (not in the reference) bit-reproducible training steps: both pooling backwards sum each source
                                # row's gradients in ascending query order over a reverse index of the kept rows' lists (no float
                                # atomics; ops._pool_bwd_raw), ops.gather_rows's backward takes its gather form, and under device
                                # draws (step_draws) the heads' Dropout mask is a keyed draw (ops.dropout_keyed) instead of a draw
                                # on torch's device generator.  Read when a call is issued: a captured graph keeps the form it
                                # was captured with.  DESIGN.md section 8g
        prop_sym_cd_w=0.0,      # (not in the reference) weight of 'Prop_sym_cd', a Chamfer term between the reconstruction and the
                                # mirrored observed cloud AS SETS (losses.prop_rot_loss, ops.recon_chamfer), beside the point-by-point
                                # L1 of 'Prop_sym_recon': 0 -- the reference's 19 terms, the key absent -- or > 0 -- a 20th term
                                # with an ordered, atomic-free backward.  No accuracy claim.  DESIGN.md section 8h
    )

    def __init__(self):
        self.__dict__.update(self._defaults)

    def reset(self):
        self.__dict__.clear()
        self.__dict__.update(self._defaults)


FLAGS = _Flags()
