"""CPU: the reference's command lines through `train.py --print-config` -- the five of GA/README.md (with --aug-repeats 3
--cooldown-epochs 10 added: both are GA/train.py's defaults) and the seven flag sets of MAP/train_with_script.py, typed in below as
the reference has them.  Each runs as a child process that ends before a model is created or a device touched and prints the
settings it resolved to as one JSON line.

The folders hold files of tests/golden/jpeg_pil.npz under many names (nothing is decoded here, the files are only listed): the GA
folder 256 of them, so that timm's selected_round of 256 keeps one round; the MAP folder 12 distinct files 25 times over, because
the recipes' batches of 64 .. 256 need that many files for one full batch, run with --selected-round 0."""
import json
import os
import subprocess
import sys

import pytest

import _jpeg_ref as J
from conftest import GOLDEN, ROOT


def _folder(root, n, classes=2):
    files = [c for c in J.load_golden(os.path.join(GOLDEN, 'jpeg_pil.npz'))[0]
             if c['kind'] == 'ok' and c['name'].startswith(('64x80', '37x53', '48x31', '17x33'))][:12]
    assert len(files) == 12
    for k in range(n):
        c = files[k % 12]
        d = os.path.join(root, f'class{k % classes}')
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f'{c["name"]}_{k // 12}.jpg'), 'wb') as f:
            f.write(c['data'])


@pytest.fixture(scope='module')
def ga_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp('ga')
    _folder(os.path.join(root, 'train'), 256)
    _folder(os.path.join(root, 'validation'), 12)
    return str(root)


@pytest.fixture(scope='module')
def map_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp('map')
    _folder(os.path.join(root, 'train'), 300)
    _folder(os.path.join(root, 'validation'), 12)
    return str(root)


def _print_config(argv, ok=True):
    r = subprocess.run([sys.executable, 'train.py'] + argv + ['--print-config'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    if not ok:
        return r, r.stdout + r.stderr
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    assert 'Model ' not in r.stdout + r.stderr                     # 'Model %s created' is logged once a model exists
    return r, json.loads(lines[0])


# GA/README.md: the training command of every model, after `train.py your_imageNet_root`
GA_COMMON = ('-b 128 --grad-accumulation 4 --smoothing 0.1 --bce-loss --opt lamb --opt-eps 1e-8 --momentum 0.8 --weight-decay 0.05 --sched '
             'cosine --epochs 300 --lr {lr} --warmup-lr 1e-6 --sched cosine -j 8 --amp --channels-last --model {model} --GA_lam -0.8 '
             '--drop-path {dp}')
GA_LINES = [('ga_convnext_tiny', '5e-3', '.2'), ('ga_convnext_small', '5e-3', '.4'), ('ga_convnext_base', '5e-3', '.5'),
            ('ga_CSWin_64_12211_tiny_224', '2e-3', '.2'), ('ga_CSWin_64_24322_small_224', '2e-3', '.4')]


@pytest.mark.parametrize('model,lr,dp', GA_LINES)
def test_ga_readme_lines_resolve(model, lr, dp, ga_dir):
    argv = [ga_dir] + GA_COMMON.format(model=model, lr=lr, dp=dp).split() + ['--aug-repeats', '3', '--cooldown-epochs', '10']
    _, cfg = _print_config(argv)
    assert cfg['model'] == model and cfg['aug_repeats'] == 3 and cfg['selected_round'] == 256 and cfg['grad_accumulation'] == 4
    assert cfg['epochs'] == 310 and cfg['cooldown_epochs'] == 10 and cfg['crop_pct'] == 0.875 and cfg['interpolation'] == 'bicubic'
    # 256 files: one round of 256 samples = 2 batches of 128, read from 256 / 3 -> 86 distinct files
    assert cfg['train_images'] == 256 and cfg['batches_per_epoch'] == 2 and cfg['distinct_files_per_epoch'] == 86


# MAP/train_with_script.py:13-19 (setting_dict) as typed there, the dataset name replaced by the folder; the script sets --model
# from its own -m list, so each set runs here with the MAP model of that family this project has (FasterViT and MaxViT are not
# built: their flag sets are resolved for map_resnet50, the script's default -m)
MAP_RECIPES = dict(
    resnet50="--input-size 3 224 224 --test-input-size 3 224 224 --aa rand-m20-mstd0.5-inc1 --mixup .1 --cutmix 1.0 --remode pixel --reprob 0.25 --crop-pct 0.95 --drop-path 0.1 --drop 0.1 --smoothing 0.1 --bce-loss --opt lamb --weight-decay .02 --sched cosine --epochs 300 --lr 5e-3 --warmup-lr 1e-6 -b 128 -j 8 --channels-last --amp -tb 1024 --pin-mem --aug-repeats 3 --log-wandb",
    pit_s="--model vit_small_patch16_224 --aa rand-m9-mstd0.5-inc1 --mixup .8 --cutmix 1.0 --aug-repeats 3 --remode pixel --reprob 0.25 --drop-path .1 --opt adamw --weight-decay .05 --sched cosine --epochs 300 --lr 1e-3 --warmup-lr 1e-6 -b 256 -tb 1024 -j 16 --amp --channels-last --log-wandb --pin-mem",
    convnext_tiny="--drop-path .1 -b 128 -tb 1024 --smoothing 0.1 --bce-loss --opt lamb --opt-eps 1e-8 --momentum 0.8 --weight-decay 0.05 --sched cosine --epochs 300 --lr 5e-3 --warmup-lr 1e-6 --crop-pct 0.875 --aa rand-m9-mstd0.5-inc1 --mixup .8 --cutmix 1.0 --remode pixel --reprob 0.25 --sched cosine -j 8 --amp --channels-last --model-ema --model-ema-decay 0.9999 --aug-repeats 3 --log-wandb",
    convnext_small="--drop-path .4 -b 128 -tb 1024 --smoothing 0.1 --bce-loss --opt lamb --opt-eps 1e-8 --momentum 0.8 --weight-decay 0.05 --sched cosine --epochs 300 --lr 5e-3 --warmup-lr 1e-6 --crop-pct 0.875 --aa rand-m9-mstd0.5-inc1 --mixup .8 --cutmix 1.0 --remode pixel --reprob 0.25 --sched cosine -j 8 --amp --channels-last --model-ema --model-ema-decay 0.9999 --aug-repeats 3 --log-wandb",
    faster_vit_3="--drop-path .3 -b 128 -tb 4096 --aug-repeat 3 --opt lamb --opt-eps 1e-8 --momentum 0.9 --weight-decay 0.05 --sched cosine --warmup-epochs 35 --epochs 300 --lr 5e-3 --warmup-lr 1e-6 --min-lr 5e-6 --crop-pct 0.95 --aa rand-m15-mstd0.5-inc1 --mixup .8 --cutmix 1.0 --remode pixel --reprob 0.25 --smoothing 0.1 --sched cosine -j 8 --amp --channels-last --log-wandb --clip-grad 5.0",
    maxvit_tiny="--model maxvit_tiny_tf_224 --aug-repeat 3 --aa rand-m15-mstd0.5-inc1 --mixup .8 --cutmix 1.0 --remode pixel --reprob 0.25 --drop-path .2 --opt lamb --bce-loss --weight-decay .05 --sched cosine --epochs 300 --lr 8e-3 --warmup-lr 1e-6 --warmup-epoch 30 --min-lr 1e-5 -b 64 -tb 4096 --smoothing 0.1 --clip-grad 1.0 -j 8 --amp --pin-mem --channels-last --log-wandb --project-name mmcap",
    mobilenet_v1="--input-size 3 160 160 --test-input-size 3 224 224 --aa rand-m7-mstd0.5-inc1 --mixup .1 --cutmix 1.0 --aug-repeats 0 --remode pixel --reprob 0.0 --crop-pct 0.95 --drop-path 0.05 --smoothing 0.0 --bce-loss --opt lamb --weight-decay .02 --sched cosine --epochs 100 --lr 5e-3 --warmup-lr 1e-6 -b 512 -j 16 --channels-last --amp -tb 1024 --pin-mem --log-wandb",
)
# recipe -> (model, batch, grad_accumulation = tb // batch on one rank, crop_pct)
MAP_EXPECT = dict(resnet50=('map_resnet50', 128, 8, 0.95), pit_s=('map_pit_s', 256, 4, 0.875), convnext_tiny=('map_convnext_tiny', 128, 8, 0.875),
                  convnext_small=('map_convnext_small', 128, 8, 0.875), faster_vit_3=('map_resnet50', 128, 32, 0.95),
                  maxvit_tiny=('map_resnet50', 64, 64, 0.875))


@pytest.mark.parametrize('recipe', sorted(MAP_EXPECT))
def test_map_recipes_resolve(recipe, map_dir):
    model, batch, accum, crop_pct = MAP_EXPECT[recipe]
    argv = [map_dir] + MAP_RECIPES[recipe].split() + ['--model', model, '--selected-round', '0', '--dec-lam', '-0.8']
    _, cfg = _print_config(argv)
    assert cfg['model'] == model and cfg['batch_size'] == batch and cfg['grad_accumulation'] == accum
    assert cfg['aug_repeats'] == 3 and cfg['selected_round'] == 0                 # --aug-repeat, the spelling of two recipes, too
    assert cfg['epochs'] == 300 and cfg['cooldown_epochs'] == 0 and cfg['crop_pct'] == crop_pct and cfg['interpolation'] == 'bicubic'
    assert cfg['drop'] == (0.1 if recipe == 'resnet50' else None)
    # 300 files, not rounded: 300 // batch full batches, their samples three copies each of consecutive files of the permutation
    assert cfg['train_images'] == 300 and cfg['batches_per_epoch'] == 300 // batch
    assert cfg['distinct_files_per_epoch'] == -(-(300 // batch * batch) // 3)
    if recipe == 'resnet50':                 # the reference's own default of 10 cooldown epochs: its 300-epoch recipes run 310
        _, cfg = _print_config(argv + ['--cooldown-epochs', '10'])
        assert cfg['epochs'] == 310 and cfg['cooldown_epochs'] == 10


def test_mobilenet_recipe_is_refused_by_its_input_size(map_dir):
    argv = [map_dir] + MAP_RECIPES['mobilenet_v1'].split() + ['--model', 'map_mobilenet_v1', '--selected-round', '0']
    r, out = _print_config(argv, ok=False)
    assert r.returncode != 0 and '--input-size 3 160 160' in out and 'other sizes are not built' in out and '{' not in r.stdout
    # the evaluation size alone is the model's own: with the training size put right the set resolves (300 files: -b 4 for 75 batches)
    argv[argv.index('--input-size') + 2:argv.index('--input-size') + 4] = ['224', '224']
    _, cfg = _print_config(argv + ['-b', '4', '-tb', '1024'])
    assert cfg['aug_repeats'] == 0 and cfg['grad_accumulation'] == 256 and cfg['epochs'] == 100 and cfg['batches_per_epoch'] == 75
    r, out = _print_config(argv + ['-b', '4', '--test-input-size', '3', '256', '256'], ok=False)
    assert r.returncode != 0 and '--test-input-size 3 256 256' in out


def test_total_batch_below_one_batch_of_every_rank_is_refused(map_dir):
    r, out = _print_config([map_dir, '--model', 'mobilenet_v1', '-b', '128', '-tb', '64'], ok=False)
    assert r.returncode != 0 and '-tb 64 is less than one batch of every rank (128 x 1 rank(s))' in out
    _, cfg = _print_config([map_dir, '--model', 'mobilenet_v1', '-b', '128', '-tb', '300', '--grad-accumulation', '7'])
    assert cfg['grad_accumulation'] == 2                                        # -tb overrides --grad-accumulation, rounded down
    _, cfg = _print_config([map_dir, '--model', 'mobilenet_v1', '-b', '128', '--grad-accumulation', '7'])
    assert cfg['grad_accumulation'] == 7 and cfg['aug_repeats'] == 0 and cfg['batches_per_epoch'] == 2      # today's defaults


def test_small_folder_under_the_default_round_is_refused_by_name(map_dir, tmp_path):
    _folder(os.path.join(tmp_path, 'train'), 12)
    _folder(os.path.join(tmp_path, 'validation'), 12)
    r, out = _print_config([str(tmp_path), '--model', 'mobilenet_v1', '-b', '4', '--aug-repeats', '3'], ok=False)
    assert r.returncode != 0 and 'selected_round 256' in out
    _, cfg = _print_config([str(tmp_path), '--model', 'mobilenet_v1', '-b', '4', '--aug-repeats', '3', '--selected-round', '0'])
    assert cfg['batches_per_epoch'] == 3 and cfg['distinct_files_per_epoch'] == 4
    _, cfg = _print_config(['--synthetic', '--model', 'mobilenet_v1', '--aug-repeats', '3'])         # accepted, no folder entries
    assert cfg['aug_repeats'] == 3 and 'batches_per_epoch' not in cfg


@pytest.mark.parametrize('name', ['mobilenet_v1', 'map_vit_small_patch16_224', 'map_vit_base_patch16_384'])
def test_model_img_size_is_the_created_models_size(name):
    import imagenet_models_amd as A
    assert A.model_img_size(name) == A.create_model(name, num_classes=10).cfg.get('img_size', 224)
    with pytest.raises(RuntimeError, match='Unknown model'):
        A.model_img_size('no_such_model')
