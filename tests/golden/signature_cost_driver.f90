!  signature_cost_driver.f90 -- TEST INFRASTRUCTURE, not product code.
!
!  A bind(C) driver over the UNMODIFIED reference modules, compiled by tests/golden/make_signature_cost.py against the module files
!  and objects the oracle recipe leaves in oracle/_ref/obj_parity (same flags: -O2 -ffp-contract=off).  Two entries:
!    sc_fn    mwd_cost::signature, MWD_COST_DIFF::SIGNATURE_B (res_b = 1) and SIGNATURE_D on one series
!             (smash/solver/optimize/mwd_cost.f90:772-970, smash/solver/forward/forward_db.f90:4501-4926)
!    sc_run   mw_forward::forward / forward_b / forward_d with input_data%mean_prcp and setup%optimize%mask_event filled, which
!             oracle/ref/ref_capi.f90 has no arguments for, and COMPUTE_JOBS_B on the forward run's discharge for output_b%qsim
!
!  This file is ours; it contains no reference source text.  Nothing compiled from it is committed.

module signature_cost_driver

    use iso_c_binding
    use md_constant
    use mwd_setup
    use mwd_mesh
    use mwd_input_data
    use mwd_parameters
    use mwd_states
    use mwd_output
    use mwd_parameters_manipulation
    use mwd_states_manipulation
    use mw_forward, only: forward, forward_b, forward_d
    use mwd_cost, only: signature
    use mwd_cost_diff, only: signature_b, signature_d, compute_jobs_b
    use mwd_output_diff, only: OutputDiffSide => OUTPUTDT, OUTPUTDT_DIFF

    implicit none

contains

    function crit_name(code) result(s)
        integer, intent(in) :: code
        character(20) :: s
        select case (code)
        case (1); s = "nse"
        case (2); s = "kge"
        case (3); s = "kge2"
        case (4); s = "se"
        case (5); s = "rmse"
        case (6); s = "logarithmic"
        case (7); s = "Crc"
        case (8); s = "Cfp2"
        case (9); s = "Cfp10"
        case (10); s = "Cfp50"
        case (11); s = "Cfp90"
        case (12); s = "Epf"
        case (13); s = "Elt"
        case (14); s = "Erc"
        case default; s = "..."
        end select
    end function crit_name

    !  one series of n steps; qs_b comes back as SIGNATURE_B leaves it from zeros with res_b = 1
    subroutine sc_fn(n, code, po, qo, qs, mask_event, qs_d, res, qs_b, res_d) bind(C, name="sc_fn")

        integer(c_int), intent(in), value :: n, code
        real(c_float), intent(in) :: po(n), qo(n), qs(n), qs_d(n)
        integer(c_int), intent(in) :: mask_event(n)
        real(c_float), intent(inout) :: res, qs_b(n), res_d

        real(sp) :: rb, r2
        character(20) :: nm

        nm = crit_name(code)
        res = signature(po, qo, qs, mask_event, trim(nm))
        qs_b = 0._sp
        rb = 1._sp
        call signature_b(po, qo, qs, qs_b, mask_event, trim(nm), rb)
        res_d = signature_d(po, qo, qs, qs_d, mask_event, trim(nm), r2)

    end subroutine sc_fn

    !  icfg = (structure 1..5; nrow; ncol; nt; ng; optimize_start_step; njf; mode 0 forward, 1 forward_b, 3 forward_d)
    !  rcfg = (dt; dx; cost_b)
    !  arrays column-major as the reference holds them, path and gauge_pos 1-based; params / states the (nrow, ncol, GNP / GNS) packings
    !  mode 0 also fills qsim_b = output_b%qsim of COMPUTE_JOBS_B (jobs_b = 1) on the run's discharge
    subroutine sc_run(icfg, rcfg, flwdir, flwacc, path, active_cell, gauge_pos, area, prcp, pet, qobs, mean_prcp, mask_event, &
    & params, states, wgauge, jobs_codes, wjobs, params_d, states_d, &
    & qsim, costs, params_b, states_b, qsim_b, qsim_d, cost_d) bind(C, name="sc_run")

        integer(c_int), intent(in) :: icfg(8)
        real(c_float), intent(in) :: rcfg(3)
        integer(c_int), intent(in) :: flwdir(icfg(2), icfg(3)), flwacc(icfg(2), icfg(3))
        integer(c_int), intent(in) :: path(2, icfg(2)*icfg(3)), active_cell(icfg(2), icfg(3))
        integer(c_int), intent(in) :: gauge_pos(icfg(5), 2)
        real(c_float), intent(in) :: area(icfg(5))
        real(c_float), intent(in) :: prcp(icfg(2), icfg(3), icfg(4)), pet(icfg(2), icfg(3), icfg(4))
        real(c_float), intent(in) :: qobs(icfg(5), icfg(4)), mean_prcp(icfg(5), icfg(4))
        integer(c_int), intent(in) :: mask_event(icfg(5), icfg(4))
        real(c_float), intent(in) :: params(icfg(2), icfg(3), GNP), states(icfg(2), icfg(3), GNS)
        real(c_float), intent(in) :: wgauge(icfg(5))
        integer(c_int), intent(in) :: jobs_codes(icfg(7))
        real(c_float), intent(in) :: wjobs(icfg(7))
        real(c_float), intent(in) :: params_d(icfg(2), icfg(3), GNP), states_d(icfg(2), icfg(3), GNS)
        real(c_float), intent(inout) :: qsim(icfg(5), icfg(4)), costs(3)
        real(c_float), intent(inout) :: params_b(icfg(2), icfg(3), GNP), states_b(icfg(2), icfg(3), GNS)
        real(c_float), intent(inout) :: qsim_b(icfg(5), icfg(4)), qsim_d(icfg(5), icfg(4)), cost_d

        type(SetupDT) :: setup
        type(MeshDT) :: mesh
        type(Input_DataDT) :: input_data
        type(ParametersDT) :: p, p_b, p_bgd, p_bgd_b, p_d
        type(StatesDT) :: s, s_b, s_bgd, s_bgd_b, s_d
        type(OutputDT) :: output, output_b, output_d
        type(OutputDiffSide) :: out_side
        type(OUTPUTDT_DIFF) :: out_side_b
        real(sp) :: cost, cost_b, cd, jobs, jobs_b
        integer :: nrow, ncol, nt, ng, njf, j

        nrow = icfg(2); ncol = icfg(3); nt = icfg(4); ng = icfg(5); njf = icfg(7)
        select case (icfg(1))
        case (1); setup%structure = "gr-a"
        case (2); setup%structure = "gr-b"
        case (3); setup%structure = "gr-c"
        case (4); setup%structure = "gr-d"
        case (5); setup%structure = "vic-a"
        end select
        setup%dt = rcfg(1)
        setup%ntime_step = nt
        setup%mean_forcing = .true.
        call SetupDT_initialise(setup, 0, ng)

        call MeshDT_initialise(mesh, setup, nrow, ncol, ng)
        mesh%dx = rcfg(2)
        mesh%flwdir = flwdir
        mesh%flwacc = flwacc
        mesh%path = path
        mesh%active_cell = active_cell
        mesh%nac = count(active_cell .eq. 1)
        mesh%gauge_pos = gauge_pos
        mesh%area = area

        call Input_DataDT_initialise(input_data, setup, mesh)
        input_data%qobs = qobs
        input_data%prcp = prcp
        input_data%pet = pet
        input_data%mean_prcp = mean_prcp

        call ParametersDT_initialise(p, mesh)
        call ParametersDT_initialise(p_b, mesh)
        call ParametersDT_initialise(p_bgd, mesh)
        call ParametersDT_initialise(p_bgd_b, mesh)
        call ParametersDT_initialise(p_d, mesh)
        call StatesDT_initialise(s, mesh)
        call StatesDT_initialise(s_b, mesh)
        call StatesDT_initialise(s_bgd, mesh)
        call StatesDT_initialise(s_bgd_b, mesh)
        call StatesDT_initialise(s_d, mesh)
        call OutputDT_initialise(output, setup, mesh)
        call OutputDT_initialise(output_b, setup, mesh)
        call OutputDT_initialise(output_d, setup, mesh)

        setup%optimize%denormalize_forward = .false.
        setup%optimize%optimize_start_step = icfg(6)
        setup%optimize%njf = njf
        setup%optimize%njr = 0
        deallocate (setup%optimize%jobs_fun, setup%optimize%wjobs_fun)
        deallocate (setup%optimize%jreg_fun, setup%optimize%wjreg_fun)
        allocate (setup%optimize%jobs_fun(njf), setup%optimize%wjobs_fun(njf))
        allocate (setup%optimize%jreg_fun(0), setup%optimize%wjreg_fun(0))
        do j = 1, njf
            setup%optimize%jobs_fun(j) = crit_name(jobs_codes(j))
            setup%optimize%wjobs_fun(j) = wjobs(j)
        end do
        setup%optimize%wjreg = 0._sp
        setup%optimize%wgauge = wgauge
        setup%optimize%mask_event = mask_event

        call set_parameters(mesh, p, params)
        call set_parameters(mesh, p_bgd, params)
        call set_states(mesh, s, states)
        call set_states(mesh, s_bgd, states)

        cost = 0._sp
        cost_b = rcfg(3)
        if (icfg(8) .eq. 0) then
            call forward(setup, mesh, input_data, p, p_bgd, s, s_bgd, output, cost)
            allocate (out_side%qsim(ng, nt), out_side_b%qsim(ng, nt))
            out_side%qsim = output%qsim
            out_side_b%qsim = 0._sp
            jobs = 0._sp
            jobs_b = 1._sp
            call compute_jobs_b(setup, mesh, input_data, out_side, out_side_b, jobs, jobs_b)
            qsim_b = out_side_b%qsim
        else if (icfg(8) .eq. 1) then
            call forward_b(setup, mesh, input_data, p, p_b, p_bgd, p_bgd_b, s, s_b, s_bgd, s_bgd_b, output, output_b, cost, cost_b)
            call get_parameters(mesh, p_b, params_b)
            call get_states(mesh, s_b, states_b)
        else
            call set_parameters(mesh, p_d, params_d)
            call set_states(mesh, s_d, states_d)
            call set_parameters(mesh, p_bgd_b, params_d)
            call set_states(mesh, s_bgd_b, states_d)
            cd = 0._sp
            call forward_d(setup, mesh, input_data, p, p_d, p_bgd, p_bgd_b, s, s_d, s_bgd, s_bgd_b, output, output_d, cost, cd)
            cost_d = cd
            qsim_d = output_d%qsim
        end if
        qsim = output%qsim
        costs(1) = cost
        costs(2) = output%cost_jobs
        costs(3) = output%cost_jreg

    end subroutine sc_run

end module signature_cost_driver
