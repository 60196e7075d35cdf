"""CPU: the two diced-inference entry scripts take one command line (neuroclear_amd/dice_cli.py).  neuroclear_amd.infer_dice2d builds the parser
of neuroclear_amd.test_dice with its own defaults for --image_dimension and --dice_size and adds --nbatch; every other flag, with its default, is the same."""


def _options(parser):
    return {a.option_strings[0]: (tuple(a.option_strings), a.default, a.nargs, a.type, a.required, type(a).__name__)
            for a in parser._actions if a.option_strings and a.dest != 'help'}


def test_the_two_parsers_accept_the_same_flags():
    from neuroclear_amd import dice_cli, infer_dice2d, test_dice
    assert test_dice.build_parser is dice_cli.build_parser     # what test_dice.main parses with
    o3, o2 = _options(test_dice.build_parser()), _options(infer_dice2d.build_parser())
    assert set(o2) - set(o3) == {'--nbatch'} and set(o3) - set(o2) == set()
    own = {'--image_dimension', '--dice_size'}
    assert {k for k in o3 if o3[k] != o2[k]} == own
    assert o3['--image_dimension'][1] == 3 and o2['--image_dimension'][1] == 2
    assert o3['--dice_size'][1] == [120, 120, 120] and o2['--dice_size'][1] == [120, 120]
    for k in own:     # only the default differs
        assert o3[k][0] == o2[k][0] and o3[k][2:] == o2[k][2:]
    assert len(o3) == 33 and o2['--nbatch'][1] == 8
    # ... and the parsed namespaces differ in those names alone
    n3, n2 = vars(test_dice.build_parser().parse_args(['--dataroot', 'd'])), vars(infer_dice2d.build_parser().parse_args(['--dataroot', 'd']))
    assert {k for k in n2 if k not in n3 or n3[k] != n2[k]} == {'nbatch', 'image_dimension', 'dice_size'}
