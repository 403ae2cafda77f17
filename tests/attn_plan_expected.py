"""What test_attention_plan_host.py recorded for every case of attn_plan_cases.py (`python tests/test_attention_plan_host.py`)."""
EXPECTED = {
    'dict_cpu_hidden': {'runs': [
        {'calls': [
        ], 'error': 'pww_hip attention needs HIP tensors (got cpu); the CPU restatement lives in oracle/ and is test-only'},
    ], 'warns': [], 'kv_cache': [], 'orig_cache': {}, 'scratch': False},
    'dict_f32_context': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'dict_f32_hidden': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@#1.view+0', 'weight': 'float16[64, 64]@#2', 'k': 'float16[2, 77, 64]@#3.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@#1.view+0', 'weight': 'float16[64, 64]@#2', 'k': 'float16[2, 77, 64]@#3.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#3.view+0', 'v': 'float16[2, 77, 64]@#3.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#3')], 'orig_cache': {}, 'scratch': False},
    'dict_f32_module': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'bfloat16[2, 16, 64]@#1.view+0', 'k': 'bfloat16[2, 77, 64]@#2', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'bfloat16[2, 16, 64]@#1.view+0', 'k': 'bfloat16[2, 77, 64]@#2', 'v': 'bfloat16[2, 77, 64]@#3', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'bfloat16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['cast', 'cast', 'cast'], 'kv_cache': [(True, 'float32[2, 77, 128]@#4')], 'orig_cache': {}, 'scratch': False},
    'dict_k_bias': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#3', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [], 'orig_cache': {}, 'scratch': False},
    'dict_k_bias_lora': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 16, 64]@#1.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('lora_update', {'y': 'float16[2, 77, 64]@#2.view+0', 'x': 'float16[2, 77, 32]@context', 'layer_stack': "stack('to_k',)", 'state': 'lora-state', 'n_seg': 1}),
            ('lora_update', {'y': 'float16[2, 77, 64]@#3', 'x': 'float16[2, 77, 32]@context', 'layer_stack': "stack('to_v',)", 'state': 'lora-state', 'n_seg': 1}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@lora_update.out~2', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@lora_update.out~2', 'v': 'float16[2, 77, 64]@#3', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [], 'orig_cache': {}, 'scratch': False},
    'dict_q_bias': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'dict_second_call': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0~2', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1~2'}),
        ], 'out': 'float16[2, 16, 64]@attention.out~2', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'dict_second_call_lora': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 77, 128]@#1', 'x': 'float16[2, 77, 32]@context.view+0', 'layer_stack': "stack('to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 2}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#2.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'v': 'float16[2, 77, 64]@#1.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
        {'calls': [
            ('lora_update', {'y': 'float16[2, 16, 64]@#3.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@lora_update.out~2', 'k': 'float16[2, 77, 64]@#1.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out~2', 'k': 'float16[2, 77, 64]@#1.view+0', 'v': 'float16[2, 77, 64]@#1.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out~2'}),
        ], 'out': 'float16[2, 16, 64]@attention.out~2', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#1')], 'orig_cache': {}, 'scratch': False},
    'dict_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_absmax': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 5, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 5, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_bare_stat': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_cw': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_cw_tensor_sigma': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_forced': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_handmade': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_head': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': None, 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_head_tensor_sigma': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_max': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_max_qp0': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_max_qproj_unsupported': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@#3.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#3.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_max_tensor_sigma': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_mean': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 3, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 3, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_mean_qp0': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 3, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 3, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_qk': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float16[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_row': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 4, 'scope': 2, 'scalar': 0.415888, 'gate': None, 'parts': None, 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_std': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 4, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 4, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_std_qp0': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 4, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 4, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'f_zero_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'fused_cross': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'fused_cross_154': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'fused_cross_cw_slots': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': 'FusedScratch', 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': True},
    'fused_cross_forced': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'fused_cross_qp0': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': 'FusedScratch', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': True},
    'fused_cross_second_call': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': 'FusedScratch', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#3.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': 'FusedScratch', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out~2', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': True},
    'gate_gated_cw': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_cw_tensor_sigma': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_head': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate'}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': 'float32[2]@gate', 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_max': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate', 'gated': 1}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 1, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_max_154': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate', 'gated': 1}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 1, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_max_qproj': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate'}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 1, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_row': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 4, 'scope': 2, 'scalar': 0.415888, 'gate': 'float32[2]@gate', 'parts': None, 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': 'float32[2]@gate', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_gated_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_negative_cw': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_negative_cw_tensor_sigma': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_negative_head': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate'}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': 'float32[2]@gate', 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_negative_max': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate', 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_negative_row': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 4, 'scope': 2, 'scalar': 0.415888, 'gate': 'float32[2]@gate', 'parts': None, 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_negative_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': 'float32[2]@gate', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_negative_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_rows_head': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate'}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': 'float32[2]@gate', 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_rows_max': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate', 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_rows_row': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 4, 'scope': 2, 'scalar': 0.415888, 'gate': 'float32[2]@gate', 'parts': None, 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_rows_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': 'float32[2]@gate', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'gate_rows_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_cw_slots_128': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'v': 'float16[2, 128, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 128]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 128]@map', (4, 16, 128), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 128, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_cw_slots_129': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 129, 64]@#2.view+0', 'v': 'float16[2, 129, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 129]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 129]@map', (4, 16, 129), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 129, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_cw_slots_154': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 154]@map', (4, 16, 154), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_cw_slots_256': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 256, 64]@#2.view+0', 'v': 'float16[2, 256, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 256]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 256]@map', (4, 16, 256), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 256, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_cw_slots_257': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'v': 'float16[2, 257, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 257]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 257]@map', (4, 16, 257), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 257, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_cw_slots_77': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_forced_128': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'v': 'float16[2, 128, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 128]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 128, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_forced_154': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_forced_257': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'v': 'float16[2, 257, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 257]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 257, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_head_128': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'v': 'float16[2, 128, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 128]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': None, 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 128, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_head_129': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 129, 64]@#2.view+0', 'v': 'float16[2, 129, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 129]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 129, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_128': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 128, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 128, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 128, 64]@#2.view+0', 'v': 'float16[2, 128, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 128]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 128, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_129': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 129, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 129, 64]@#2.view+0', 'v': 'float16[2, 129, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 129]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 129, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_154': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_256': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 256, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 256, 64]@#2.view+0', 'v': 'float16[2, 256, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 256]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 256, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_257': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'v': 'float16[2, 257, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 257]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 257, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_77': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_qp0_128': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'v': 'float16[2, 128, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 128]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 128, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_max_qp0_129': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 129, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 129, 64]@#2.view+0', 'v': 'float16[2, 129, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 129]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 129, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_row_128': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 128, 64]@#2.view+0', 'v': 'float16[2, 128, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 128]@map', 'kind': 4, 'scope': 2, 'scalar': 0.415888, 'gate': None, 'parts': None, 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 128, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_row_129': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 129, 64]@#2.view+0', 'v': 'float16[2, 129, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 129]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 129, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_tensor_154': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@#3', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'keys_zero_257': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'v': 'float16[2, 257, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 257, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'lazy_w_off_cw': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'lazy_w_off_max': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[2, 1, 16, 77]@#3', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'lazy_w_off_zero_slots': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.0,), 'sites': [(-1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'lora_and_out_self': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 16, 192]@#1.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q', 'to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 3}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 16, 64]@#1.view+64', 'v': 'float16[2, 16, 64]@#1.view+128', 'heads': 2, 'scale': 0.176777}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#2.view+0', 'x': 'float16[2, 16, 64]@attention.out', 'layer_stack': "stack('to_out.0',)", 'state': 'lora-state', 'n_seg': 1}),
        ], 'out': 'float16[2, 16, 64]@lora_update.out~2', 'projected': None},
    ], 'warns': []},
    'lora_head': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 77, 128]@#1', 'x': 'float16[2, 77, 32]@context.view+0', 'layer_stack': "stack('to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 2}),
            ('scoped_available', {}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#2.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'v': 'float16[2, 77, 64]@#1.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': None, 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#1')], 'orig_cache': {}, 'scratch': False},
    'lora_max_qproj_all': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 77, 128]@#1', 'x': 'float16[2, 77, 32]@context.view+0', 'layer_stack': "stack('to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 2}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#2.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'v': 'float16[2, 77, 64]@#1.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#1')], 'orig_cache': {}, 'scratch': False},
    'lora_to_out': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 77, 128]@#1', 'x': 'float16[2, 77, 32]@context.view+0', 'layer_stack': "stack('to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 2}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#2.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'v': 'float16[2, 77, 64]@#1.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#3.view+0', 'x': 'float16[2, 16, 64]@attention.out', 'layer_stack': "stack('to_out.0',)", 'state': 'lora-state', 'n_seg': 1}),
        ], 'out': 'float16[2, 16, 64]@lora_update.out~2', 'projected': None},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#1')], 'orig_cache': {}, 'scratch': False},
    'lora_zero_full_context': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 77, 128]@#1', 'x': 'float16[2, 77, 32]@context', 'layer_stack': "stack('to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 2}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#2.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#1.view+0', 'v': 'float16[2, 77, 64]@#1.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#1')], 'orig_cache': {}, 'scratch': False},
    'map_bias_cols': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 40, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'map_bias_cols_gated_154': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate', 'gated': 1}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 40, 'compact': None, 'gated': 1, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'map_compact': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': ('float32[16, 4]@compact_w', 'int32[4]@compact_idx'), 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'map_compact_cw': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'map_compact_other': {'runs': [
        {'calls': [
            ('resize_tokens', {'w_orig': 'float32[8, 8, 77]@orig', 'n_tokens': 16}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@resize_tokens.out', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {16: 'float32[16, 77]@resize_tokens.out'}, 'scratch': False},
    'map_compact_qproj': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': ('float32[16, 4]@compact_w', 'int32[4]@compact_idx'), 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'map_orig': {'runs': [
        {'calls': [
            ('resize_tokens', {'w_orig': 'float32[8, 8, 77]@orig', 'n_tokens': 16}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@resize_tokens.out', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {16: 'float32[16, 77]@resize_tokens.out'}, 'scratch': False},
    'map_orig0': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'map_orig0_slots': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.0,), 'sites': [(-1, 0, (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'map_orig4': {'runs': [
        {'calls': [
            ('resize_tokens', {'w_orig': 'float32[8, 8, 77]@orig.view+0', 'n_tokens': 16}),
            ('resize_tokens', {'w_orig': 'float32[8, 8, 77]@orig.view+4928', 'n_tokens': 16}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[2, 1, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {16: 'float32[2, 1, 16, 77]@#3.view+0'}, 'scratch': False},
    'map_orig_second_call': {'runs': [
        {'calls': [
            ('resize_tokens', {'w_orig': 'float32[8, 8, 77]@orig', 'n_tokens': 16}),
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@resize_tokens.out', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#3.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#3.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@resize_tokens.out', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out~2'}),
        ], 'out': 'float16[2, 16, 64]@attention.out~2', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {16: 'float32[16, 77]@resize_tokens.out'}, 'scratch': False},
    'map_orig_slots': {'runs': [
        {'calls': [
            ('resize_tokens', {'w_orig': 'float32[8, 8, 77]@orig', 'n_tokens': 16}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@resize_tokens.out', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 77]@resize_tokens.out', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {16: 'float32[16, 77]@resize_tokens.out'}, 'scratch': False},
    'qproj_0_c1280': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 1280]@#1.view+0', 'k': 'float16[2, 77, 1280]@#2.view+0', 'heads': 8, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 1280]@#1.view+0', 'k': 'float16[2, 77, 1280]@#2.view+0', 'v': 'float16[2, 77, 1280]@#2.view+1280', 'heads': 8, 'scale': 0.0790569, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 1280]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 2560]@#2')], 'orig_cache': {}, 'scratch': False},
    'qproj_0_c320': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 320]@#1.view+0', 'k': 'float16[2, 77, 320]@#2.view+0', 'heads': 8, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 320]@#1.view+0', 'k': 'float16[2, 77, 320]@#2.view+0', 'v': 'float16[2, 77, 320]@#2.view+320', 'heads': 8, 'scale': 0.158114, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 320]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 640]@#2')], 'orig_cache': {}, 'scratch': False},
    'qproj_1_c1280': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 1280]@#1.view+0', 'k': 'float16[2, 77, 1280]@#2.view+0', 'heads': 8, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 1280]@#1.view+0', 'k': 'float16[2, 77, 1280]@#2.view+0', 'v': 'float16[2, 77, 1280]@#2.view+1280', 'heads': 8, 'scale': 0.0790569, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 1280]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 2560]@#2')], 'orig_cache': {}, 'scratch': False},
    'qproj_1_c320': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 320]@hidden', 'weight': 'float16[320, 320]@#1', 'k': 'float16[2, 77, 320]@#2.view+0', 'heads': 8}),
            ('qproj_stat', {'x': 'float16[2, 16, 320]@hidden', 'weight': 'float16[320, 320]@#1', 'k': 'float16[2, 77, 320]@#2.view+0', 'heads': 8, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 320]@qproj_stat.out0', 'k': 'float16[2, 77, 320]@#2.view+0', 'v': 'float16[2, 77, 320]@#2.view+320', 'heads': 8, 'scale': 0.158114, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 320]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 640]@#2')], 'orig_cache': {}, 'scratch': False},
    'qproj_all_c1280': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 1280]@hidden', 'weight': 'float16[1280, 1280]@#1', 'k': 'float16[2, 77, 1280]@#2.view+0', 'heads': 8}),
            ('qproj_stat', {'x': 'float16[2, 16, 1280]@hidden', 'weight': 'float16[1280, 1280]@#1', 'k': 'float16[2, 77, 1280]@#2.view+0', 'heads': 8, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 1280]@qproj_stat.out0', 'k': 'float16[2, 77, 1280]@#2.view+0', 'v': 'float16[2, 77, 1280]@#2.view+1280', 'heads': 8, 'scale': 0.0790569, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 1280]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 2560]@#2')], 'orig_cache': {}, 'scratch': False},
    'qproj_all_c320': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 320]@hidden', 'weight': 'float16[320, 320]@#1', 'k': 'float16[2, 77, 320]@#2.view+0', 'heads': 8}),
            ('qproj_stat', {'x': 'float16[2, 16, 320]@hidden', 'weight': 'float16[320, 320]@#1', 'k': 'float16[2, 77, 320]@#2.view+0', 'heads': 8, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 320]@qproj_stat.out0', 'k': 'float16[2, 77, 320]@#2.view+0', 'v': 'float16[2, 77, 320]@#2.view+320', 'heads': 8, 'scale': 0.158114, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 320]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 640]@#2')], 'orig_cache': {}, 'scratch': False},
    'qproj_all_cw_slots': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_fused': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': 'FusedScratch', 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['record_fused'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': True},
    'rec_fused_qproj': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@#3', 1, 0.415888), 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_gated_parts': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate', 'gated': 1}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 1, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': ('float64[2, 4]@#3', 1, 0.415888), 'coeff_dev': None, 'images': 1, 'out': 'float32[1, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_head': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_long': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@#3', 1, 0.415888), 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 154]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_long_256': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 256, 64]@#2.view+0', 'heads': 2, 'kind': 4, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 256, 64]@#2.view+0', 'v': 'float16[2, 256, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 256]@map', 'bias_coeff': None, 'stat': (None, 4, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 256, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 256]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@#3', 4, 0.415888), 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 256]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 256, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_long_none': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'stats_out': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'coeff_dev': 'float32[1]@slots.view+0', 'images': 0, 'out': 'float32[2, 16, 154]@#3.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 154]@map', (4, 16, 154), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_muted_long': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_muted_parts': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_muted_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_negative_parts': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': 'float32[2]@gate', 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@gate', 'stat': ('float64[2, 4]@#3', 1, 0.415888), 'coeff_dev': None, 'images': 1, 'out': 'float32[1, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_parts': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@#3', 1, 0.415888), 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_parts_none': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'stats_out': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'coeff_dev': 'float32[1]@slots.view+0', 'images': 0, 'out': 'float32[2, 16, 77]@#3.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_parts_qproj': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@#3', 1, 0.415888), 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_parts_slots': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'stats_out': 'float64[2, 4]@#3', 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@#3', 1, 0.415888), 'coeff_dev': 'float32[1]@slots.view+0', 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_plain': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_plain_python_coeff': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3', 'stat': None, 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_refused_257': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'v': 'float16[2, 257, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 257]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['record_keys'], 'kv_cache': [(True, 'float16[2, 257, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_refused_257_none': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 257, 64]@#2.view+0', 'v': 'float16[2, 257, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 257]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'stats_out': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['record_keys'], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 257]@map', (4, 16, 257), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 257, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_stat': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#3.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': None, 'stat': None, 'scratch': None, 'stats_out': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': None, 'stat': None, 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#4.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_tensor_ctx': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'rec_to_out': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_out_supported', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'bias_cols': 0}),
            ('attention_out', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'weight_bias': 'float16[64]@to_out.bias', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'parts': 'float64[2, 3, 4]@qproj_stat.out1', 'coeff_dev': None, 'bias_cols': 0, 'gated': 0}),
        ], 'out': 'float16[2, 16, 64]@attention_out.out', 'projected': True},
    ], 'warns': ['record_to_out'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'rec_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
            ('attention_probs', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'scale': 0.176777, 'bias': None, 'bias_coeff': None, 'stat': None, 'coeff_dev': None, 'images': 0, 'out': 'float32[2, 16, 77]@#3.view+0', 'accumulate': True}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'scoped_no_library': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'scoped_off_head': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'scoped_off_row': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'scoped_out_linear': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'self': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 16, 64]@#1.view+64', 'v': 'float16[2, 16, 64]@#1.view+128', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'self_f32': {'runs': [
        {'calls': [
            ('attention', {'q': 'bfloat16[2, 16, 64]@#1.view+0', 'k': 'bfloat16[2, 16, 64]@#2.view+0', 'v': 'bfloat16[2, 16, 64]@#3.view+0', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'bfloat16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['cast', 'cast', 'cast']},
    'self_lora': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 16, 192]@#1.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q', 'to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 3}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 16, 64]@#1.view+64', 'v': 'float16[2, 16, 64]@#1.view+128', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'self_q_bias': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 16, 64]@#2.view+0', 'v': 'float16[2, 16, 64]@#3.view+0', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'self_q_bias_lora': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 16, 64]@#1.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#2.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_k',)", 'state': 'lora-state', 'n_seg': 1}),
            ('lora_update', {'y': 'float16[2, 16, 64]@#3.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_v',)", 'state': 'lora-state', 'n_seg': 1}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 16, 64]@lora_update.out~2', 'v': 'float16[2, 16, 64]@lora_update.out~3', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'slots_fresh_bare_stat': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.0,), 'sites': [(-1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_cw': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_cw_tensor_sigma': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_forced': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_head': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': None, 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': 'float32[1]@slots.view+0'}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [((1, 1), 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_max': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_max_154': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(1, 'float32[16, 154]@map', (4, 16, 154), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_max_qp0': {'runs': [
        {'calls': [
            ('qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_max_second_call': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0~2', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': 'float32[1]@slots.view+1', 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1~2'}),
        ], 'out': 'float16[2, 16, 64]@attention.out~2', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 2, 'words': (0.415888, 0.415888), 'sites': [(1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16'), (1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_qk': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float16[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_row': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 4, 'scope': 2, 'scalar': 0.415888, 'gate': None, 'parts': None, 'coeff_dev': 'float32[1]@slots.view+0'}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [((4, 2), 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_tensor_ctx': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'slots_fresh_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.0,), 'sites': [(-1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_fresh_zero_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.0,), 'sites': [(-1, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_bare_stat': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_cw': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 0, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_cw_tensor_sigma': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_forced': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_head': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('scope_head_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 1, 'scope': 1, 'scalar': 0.415888, 'gate': None, 'parts': 'float64[2, 2, 3, 4]@scope_head_parts.out', 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_max': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_qk': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float16[4, 16, 77]@#3.view+0', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': ['materialize'], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_row': {'runs': [
        {'calls': [
            ('scoped_available', {}),
            ('attention_scoped', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'kind': 4, 'scope': 2, 'scalar': 0.415888, 'gate': None, 'parts': None, 'coeff_dev': None}),
        ], 'out': 'float16[2, 16, 64]@attention_scoped.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@#3', 'bias_coeff': None, 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'slots_unsupported_zero_tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'slots': {'unsupported': True, 'cursor': 0, 'words': (), 'sites': []}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'tensor': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'tensor_f32_context': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'tensor_k_bias': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#3', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'tensor_k_bias_lora': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 16, 64]@#1.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('lora_update', {'y': 'float16[2, 77, 64]@#2.view+0', 'x': 'float16[2, 77, 32]@context', 'layer_stack': "stack('to_k',)", 'state': 'lora-state', 'n_seg': 1}),
            ('lora_update', {'y': 'float16[2, 77, 64]@#3', 'x': 'float16[2, 77, 32]@context', 'layer_stack': "stack('to_v',)", 'state': 'lora-state', 'n_seg': 1}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@lora_update.out~2', 'v': 'float16[2, 77, 64]@#3', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'tensor_lora': {'runs': [
        {'calls': [
            ('lora_update', {'y': 'float16[2, 16, 64]@#1.view+0', 'x': 'float16[2, 16, 64]@hidden', 'layer_stack': "stack('to_q',)", 'state': 'lora-state', 'n_seg': 1}),
            ('lora_update', {'y': 'float16[2, 77, 128]@#2', 'x': 'float16[2, 77, 32]@context.view+0', 'layer_stack': "stack('to_k', 'to_v')", 'state': 'lora-state', 'n_seg': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@lora_update.out', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': []},
    'to_out_direct_154': {'runs': [
        {'calls': [
            ('long_qk_parts', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None, 'gated': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 154, 64]@#2.view+0', 'v': 'float16[2, 154, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 154]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@long_qk_parts.out'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 154, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_direct_cw_slots': {'runs': [
        {'calls': [
            ('attention_out_supported', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'bias_cols': 40}),
            ('attention_out', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'weight_bias': 'float16[64]@to_out.bias', 'bias_coeff': 'float32[2]@gate', 'stat': (None, 0, 0.415888), 'parts': None, 'coeff_dev': 'float32[1]@slots.view+0', 'bias_cols': 40, 'gated': 1}),
        ], 'out': 'float16[2, 16, 64]@attention_out.out', 'projected': True},
    ], 'warns': [], 'slots': {'unsupported': False, 'cursor': 1, 'words': (0.415888,), 'sites': [(0, 'float32[16, 77]@map', (4, 16, 77), 'torch.float16')]}, 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_direct_forced': {'runs': [
        {'calls': [
            ('qk_stats', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': ('float64[2, 4]@qk_stats.out', 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_direct_fused_cross': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': 'FusedScratch', 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': True},
    'to_out_direct_no': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_out_supported', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'bias_cols': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_direct_plain': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': 'float32[2]@#3.view+0', 'stat': None, 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': None}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_direct_yes': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_out_supported', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'bias_cols': 0}),
            ('attention_out', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'weight_bias': 'float16[64]@to_out.bias', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'parts': 'float64[2, 3, 4]@qproj_stat.out1', 'coeff_dev': None, 'bias_cols': 0, 'gated': 0}),
        ], 'out': 'float16[2, 16, 64]@attention_out.out', 'projected': True},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_direct_zero': {'runs': [
        {'calls': [
            ('attention', {'q': 'float16[2, 16, 64]@#1.view+0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777}),
        ], 'out': 'float16[2, 16, 64]@attention.out', 'projected': False},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_no': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_out_supported', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'bias_cols': 0}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@#3.view+0', 'projected': None},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_switch_off': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'scratch': None, 'coeff_dev': None, 'bias_cols': 0, 'compact': None, 'gated': 0, 'parts': 'float64[2, 3, 4]@qproj_stat.out1'}),
        ], 'out': 'float16[2, 16, 64]@#3.view+0', 'projected': None},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
    'to_out_yes': {'runs': [
        {'calls': [
            ('qproj_parts', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2}),
            ('qproj_stat', {'x': 'float16[2, 16, 64]@hidden', 'weight': 'float16[64, 64]@#1', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'kind': 1, 'gate': None}),
            ('attention_out_supported', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'heads': 2, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'bias_cols': 0}),
            ('attention_out', {'q': 'float16[2, 16, 64]@qproj_stat.out0', 'k': 'float16[2, 77, 64]@#2.view+0', 'v': 'float16[2, 77, 64]@#2.view+64', 'heads': 2, 'scale': 0.176777, 'bias': 'float32[16, 77]@map', 'weight': 'float16[64, 64]@to_out.weight', 'weight_bias': 'float16[64]@to_out.bias', 'bias_coeff': None, 'stat': (None, 1, 0.415888), 'parts': 'float64[2, 3, 4]@qproj_stat.out1', 'coeff_dev': None, 'bias_cols': 0, 'gated': 0}),
        ], 'out': 'float16[2, 16, 64]@attention_out.out', 'projected': None},
    ], 'warns': [], 'kv_cache': [(True, 'float16[2, 77, 128]@#2')], 'orig_cache': {}, 'scratch': False},
}
