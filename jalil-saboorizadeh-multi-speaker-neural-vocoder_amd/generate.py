"""Drop-in for the reference's generate.py (generate.py:1-346): the generation CLI that
gen.sh calls (gen.sh:56), on the device generation path.

Same arguments and defaults, the experiment-tag re-parse of --model's directory
(generate.py:122-126: 'key:value~key:value' overrides), the conditioning pipeline
(.cc + interpolated .lf0 / .gv + u/v, min-max normalisation from
npy_datasets/min_max_{ind,joint}[_static].npy, optional look-ahead), the per-file seed, the
spk_dim rule (number of symlinks in datasets_path/cond_set) and the output file name
`<results>/<tag>/samples/<ckpt>_file-<name>_spk-<id>.wav` (float32, sample_rate).

Two sampling modes:
  * --sampler torch (default): the reference's behaviour file by file -- reseed, build the
    model (same RNG consumption as the reference's init), draw Exp(1) noise from torch's CPU
    generator in the reference's order: the sample stream replays the reference's.
  * --sampler philox --batch_files true: every file of the list in ONE device call (rows =
    files x n_samples, conditioning zero-padded to the longest file, outputs trimmed to each
    file's own length -- rows never interact), noise from the on-device Philox generator.

Beyond the reference: --temperature T (default 1.0) and --top_k K (default 0 = off) set the
Generator's sampling controls for every row of every call -- the draw becomes
argmax(z - T log q) over the K largest logits; --temperature 0 is greedy (no randomness).
--top_p P (default 1.0 = off, 0 < P <= 1) cuts the draw further to the nucleus: the most
probable classes whose tempered mass reaches P.
At the defaults the run is the reference's draw, bit for bit as before.
--chunk_frames N (default 0 = the whole utterance in one call) generates N conditioning frames
per call through Generator.stream, the recurrent state carried from call to call: the same
WAV, byte for byte, with the sampler's host noise bounded by the chunk (single-process runs;
rank-sharded batches are generated whole).
--session True (with --chunk_frames, or with --batch_files True --slots) runs those chunks through
one generation session (Generator.session): the same WAVs, without each call's set-up.
--scores True (default off: the WAVs are byte for byte what they are without it) also writes
<wav name minus .wav>.scores.npy beside each WAV -- float32 (T, 2), T the file's own length: the
log-prob of each sample drawn and the entropy of the model's distribution there, in nats -- and
prints the file's bits per sample.  Rank-sharded batches are generated without scores.
"""
import argparse
import os
import random
import re
import sys

import numpy as np
import torch

from dataset import read_conditioners, write_wav
from model import Generator, Predictor, SampleRNN, bits_per_sample, shard_generate

default_params = {
    # model parameters
    'n_rnn': 1,
    'dim': 1024,
    'learn_h0': True,
    'ulaw': True,
    'q_levels': 256,
    'weight_norm': False,
    'seq_len': 1040,
    'batch_size': 128,
    'look_ahead': False,
    'qrnn': False,
    'val_frac': 0.1,
    'test_frac': 0.1,
    'cond_dim': 43,
    'norm_ind': False,
    'static_spk': False,
    # training parameters
    'sample_rate': 16000,
    'n_samples': 1,
    'sample_length': 80000,
    'seed': 77977,
    'cond': 0,
    # generator parameters
    'datasets_path': '/veu/tfgveu7/project/tcstar/',
    'cond_set': 'cond/',
    'cond_list': 'generate_cond_gina.list',
    'spk_list': 'generate_spk_gina.list',
    'sampler': 'torch',
    'batch_files': False,
    'compute_dtype': 'fp32',
    'temperature': 1.0,
    'top_k': 0,
    'top_p': 1.0,
    'chunk_frames': 0,
    'slots': 0,
    'session': False,
    'scores': False,
}


def run_generator(gen, n_seqs, sample_length, cond, spk, chunk_frames, session=False,
                  scores=False, **kw):
    """Generator.__call__, or the concatenated blocks of Generator.stream when chunk_frames is
    set (equal bit for bit), through one session when asked.  scores: returns (samples, the
    (n_seqs, T, 2) per-step scores) in place of the samples."""
    if scores:
        kw['return_scores'] = True
    if chunk_frames > 0:
        blocks = list(gen.stream(n_seqs, cond, spk, chunk_frames, session=session, **kw))
        if scores:
            return tuple(torch.cat([b[k] for b in blocks], dim=1) for k in (0, 1))
        return torch.cat(blocks, dim=1)
    return gen(n_seqs, sample_length, cond, spk, **kw)


def write_scores(wav_name, scores):
    """The (T, 2) float32 scores of one WAV beside it (<name minus .wav>.scores.npy), and its
    bits per sample on stdout."""
    scores = np.ascontiguousarray(np.asarray(scores, dtype=np.float32))
    np.save(wav_name[:-4] + '.scores.npy', scores)
    print('%s: %.4f bits per sample' % (wav_name, float(bits_per_sample(scores)[0])))


def init_random_seed(seed, cuda):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if cuda:
        torch.cuda.manual_seed(seed)


def as_type(var, target_type):
    """generate.py:53-64: re-type a tag value like the default it overrides."""
    if target_type is bool:
        return var[0] == 'T'
    if target_type is int:
        return int(var)
    if target_type is float:
        return float(var)
    if target_type is list:
        return list(map(int, var.split(',')))
    return var


def load_model(checkpoint_path):
    """generate.py:67-84."""
    m = re.match('.*ep{}-it{}'.format(r'(\d+)', r'(\d+)'), os.path.basename(checkpoint_path))
    epoch, iteration = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
    return torch.load(checkpoint_path, map_location='cpu', weights_only=True), epoch, iteration


def output_name(checkpoints_path, original_name, spk_name):
    """generate.py:99-101."""
    parts = checkpoints_path.split('/')
    return '/'.join(parts[:2]) + '/samples/' + parts[-1] + '_file-' + original_name + \
        '_spk-' + spk_name + '.wav'


def file_conditioning(stem, speaker, params):
    """generate.py:146-185: [cc | lf0 | fv | uv], normalised, optional look-ahead."""
    c, f0, fv, uv = read_conditioners(stem)
    cond = np.concatenate((c, f0, fv, uv), axis=1)
    st = '_static' if params['static_spk'] else ''
    mm = np.load('npy_datasets/min_max' + ('_ind' if params['norm_ind'] else '_joint') + st +
                 '.npy')
    lo, hi = mm[0], mm[1]
    if params['norm_ind']:
        cond = (cond - lo[speaker]) / (hi[speaker] - lo[speaker])
    else:
        cond = (cond - lo) / (hi - lo)
    if params['look_ahead']:
        nxt = np.copy(cond)
        nxt[:-1, :] = nxt[1:, :]
        cond = np.concatenate((cond, nxt), axis=1)
    return cond


def build_model(params, spk_dim, use_cuda):
    model = SampleRNN(frame_sizes=params['frame_sizes'], n_rnn=params['n_rnn'],
                      dim=params['dim'], learn_h0=params['learn_h0'],
                      q_levels=params['q_levels'], ulaw=params['ulaw'],
                      weight_norm=params['weight_norm'],
                      cond_dim=params['cond_dim'] * (1 + params['look_ahead']),
                      spk_dim=spk_dim, qrnn=params['qrnn'])
    model.compute_dtype = torch.bfloat16 if params['compute_dtype'] == 'bf16' else torch.float32
    predictor = Predictor(model)
    if use_cuda:
        model = model.cuda()
        predictor = predictor.cuda()
    state_dict, _, _ = load_model(params['model'])
    predictor.load_state_dict(state_dict)
    return model


def main(frame_sizes, **params):
    import distributed as Dd
    Dd.init()                   # torchrun: one process per GPU (no-op for a single process)
    use_cuda = torch.cuda.is_available()
    if use_cuda:
        torch.cuda.set_device(Dd.device_index())
    rank, world = Dd.rank(), Dd.world()
    params = dict(default_params, frame_sizes=frame_sizes, **params)
    # parameters encoded in the experiment directory name (generate.py:122-126)
    parts = params['model'].split('/')
    if len(parts) > 1:
        for item in parts[1].split('~'):
            kv = item.split(':')
            if len(kv) == 2 and kv[0] in params:
                params[kv[0]] = as_type(kv[1], type(params[kv[0]]))
    root = str(params['datasets_path'])
    file_names = open(root + params['cond_list']).read().splitlines()
    spk_names = open(root + params['spk_list']).read().splitlines()
    if len(spk_names) != len(file_names):
        sys.exit('Length of speaker file do not match length of conditioner file.')
    cond_dir = os.path.join(root, params['cond_set'])
    spk = np.load('npy_datasets/spk_id.npy')
    spk_dim = len([i for i in os.listdir(cond_dir) if os.path.islink(os.path.join(cond_dir, i))])
    jobs = []
    for name, spk_name in zip(file_names, spk_names):
        speaker = int(np.where(spk == spk_name)[0][0])
        original = name.split('/')[1] if '/' in name else name
        if original == '..':
            original = name.split('/')[3]
        jobs.append((cond_dir + name, speaker, original))
    if params['slots'] > 0:
        # continuous batching (Generator.serve): the files through a fixed number of rows
        if not params['batch_files']:
            sys.exit('--slots needs --batch_files True.')
        if params['sampler'] != 'philox':
            sys.exit('--slots serves with the device sampler only: pass --sampler philox.')
        if world > 1:
            sys.exit('--slots runs in a single process.')
    if params['session'] and not (params['chunk_frames'] > 0 or params['slots'] > 0):
        sys.exit('--session goes with --chunk_frames N or --slots N.')
    if params['batch_files']:
        init_random_seed(params['seed'], use_cuda)
        model = build_model(params, spk_dim, use_cuda)
        conds = [file_conditioning(stem, sp, params) for stem, sp, _ in jobs]
        n = params['n_samples']
        n_cond = max(c.shape[0] for c in conds)
        C = conds[0].shape[1]
        rows = np.zeros((len(jobs) * n, n_cond, C), dtype=np.float32)
        spks = np.zeros(len(jobs) * n, dtype=np.int64)
        for j, c in enumerate(conds):
            rows[j * n:(j + 1) * n, :c.shape[0]] = c
            spks[j * n:(j + 1) * n] = jobs[j][1]
        gen = Generator(model, use_cuda)
        ctrl = dict(temperature=params['temperature'], top_k=params['top_k'],
                    top_p=params['top_p'])
        want_scores = params['scores']
        sc = None
        if want_scores and world > 1:
            print('--scores: rank-sharded batches are generated without scores')
            want_scores = False
        if params['slots'] > 0:
            # stream ids j n + i: the Philox rows of the padded batch below
            given = {k: v for k, v in ctrl.items() if v != default_params[k]}
            reqs = [dict(cond=conds[j], spk=jobs[j][1], stream_id=j * n + i, **given)
                    for j in range(len(jobs)) for i in range(n)]
            out = np.zeros((len(rows), n_cond * model.lookback), dtype=np.float32)
            if want_scores:
                sc = np.zeros((len(rows), n_cond * model.lookback, 2), dtype=np.float32)
                for u, samples, s in gen.serve(reqs, params['slots'],
                                               params['chunk_frames'] or 32, seed=params['seed'],
                                               session=params['session'], scores=True):
                    out[u, :samples.shape[0]] = samples.numpy()
                    sc[u, :s.shape[0]] = s.numpy()
            else:
                for u, samples in gen.serve(reqs, params['slots'], params['chunk_frames'] or 32,
                                            seed=params['seed'], session=params['session']):
                    out[u, :samples.shape[0]] = samples.numpy()
        elif world > 1:
            # rank-sharded: contiguous row shards gathered at the end (rows
            # padded to a multiple of the world size); either sampler reproduces the
            # single-process stream (shard_generate)
            pad = (-len(rows)) % world
            prow = np.concatenate([rows, np.zeros((pad,) + rows.shape[1:], rows.dtype)])
            pspk = np.concatenate([spks, np.zeros(pad, spks.dtype)])
            out = shard_generate(gen, len(prow), prow, pspk, params['seed'],
                                 sampler=params['sampler'], noise_rows=len(rows),
                                 seq_len=params['sample_length'], **ctrl).numpy()[:len(rows)]
        else:
            out = run_generator(gen, len(rows), params['sample_length'], rows, spks,
                                params['chunk_frames'], session=params['session'],
                                scores=want_scores, sampler=params['sampler'],
                                seed=params['seed'], **ctrl)
            if want_scores:
                out, sc = out[0], out[1].numpy()
            out = out.numpy()
        if rank != 0:
            return
        L = model.lookback
        for j, (stem, sp, original) in enumerate(jobs):
            fname = output_name(params['model'], original, str(spk[sp]))
            for i in range(n):
                write_wav(fname, out[j * n + i, :conds[j].shape[0] * L], sr=params['sample_rate'])
                if sc is not None:
                    write_scores(fname, sc[j * n + i, :conds[j].shape[0] * L])
        return
    for j, (stem, speaker, original) in enumerate(jobs):
        if j % world != rank:       # files are independent: round-robin over the ranks
            continue
        cond = file_conditioning(stem, speaker, params)
        init_random_seed(params['seed'], use_cuda)
        model = build_model(params, spk_dim, use_cuda)
        fname = output_name(params['model'], original, str(spk[speaker]))
        print('Generating file', fname)
        gen = Generator(model, use_cuda)
        samples = run_generator(gen, params['n_samples'], params['sample_length'], cond, speaker,
                                params['chunk_frames'], session=params['session'],
                                scores=params['scores'],
                                sampler=params['sampler'], seed=params['seed'],
                                temperature=params['temperature'],
                                top_k=params['top_k'], top_p=params['top_p'])
        sc = None
        if params['scores']:
            samples, sc = samples
        samples = samples.numpy()
        for i in range(params['n_samples']):
            write_wav(fname, samples[i, :], sr=params['sample_rate'])
            if sc is not None:
                write_scores(fname, sc[i].numpy())


def parse_bool(arg):
    arg = arg.lower()
    if 'true'.startswith(arg):
        return True
    if 'false'.startswith(arg):
        return False
    raise ValueError(arg)


def build_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                argument_default=argparse.SUPPRESS)
    p.add_argument('--frame_sizes', nargs='+', type=int, required=True,
                   help='frame sizes in terms of the number of lower tier frames, '
                        'starting from the lowest RNN tier')
    p.add_argument('--model', required=True, help='model (including path)')
    for name, typ in (('n_rnn', int), ('dim', int), ('learn_h0', parse_bool),
                      ('ulaw', parse_bool), ('q_levels', int), ('seq_len', int),
                      ('batch_size', int), ('datasets_path', str), ('cond_set', str),
                      ('sample_rate', int), ('n_samples', int), ('sample_length', int),
                      ('norm_ind', parse_bool), ('look_ahead', float),
                      ('static_spk', parse_bool), ('seed', int), ('weight_norm', parse_bool),
                      ('cond_list', str), ('spk_list', str), ('sampler', str),
                      ('batch_files', parse_bool), ('compute_dtype', str),
                      ('temperature', float), ('top_k', int), ('top_p', float),
                      ('chunk_frames', int), ('slots', int), ('session', parse_bool),
                      ('scores', parse_bool)):
        p.add_argument('--' + name, type=typ)
    # gen.sh passes --results_path (generate.py has no such option; accepted and ignored)
    p.add_argument('--results_path', type=str)
    p.set_defaults(**default_params)
    return p


if __name__ == '__main__':
    args = vars(build_parser().parse_args())
    args.pop('results_path', None)
    if isinstance(args.get('look_ahead'), float):
        args['look_ahead'] = bool(args['look_ahead'])
    main(**args)
